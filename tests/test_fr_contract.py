"""fr.h on the device, one routine at a time, at the edges of its stated operand ranges (tests/fr_contract_common.py is the contract):
hz_fr_raw_ops runs ONE routine per kernel on raw limbs, in both builds of the kernels -- form 0 with HZ_FR_INLINE as every kernel of
the step has it, form 1 without it (fr_mul / fr_sqr / fr_to_canon / fr_inv out of line, as the gadget mains call them). Python
integers judge the result: congruence, normalised limbs, the stated bound -- not the present representative."""
import ctypes

import numpy as np
import pytest

import fr_contract_common as FC

FORMS = {0: "inline (HZ_FR_INLINE)", 1: "out of line"}


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", list(FC.OPS))
def test_hip_fr_routine_keeps_its_contract(hz, name, form):
    op = FC.OPS[name]
    tuples = FC.operands(name)
    out = hz.fr_raw_ops(op.code, form, FC.packed(name))
    FC.judge(op, tuples, out, "device, " + FORMS[form])
    # the wave-uniform branches: values placed on chosen lanes of chosen wavefronts (element i runs on lane i % 64)
    for label, sc in FC.wave_scenarios(name):
        out = hz.fr_raw_ops(op.code, form, FC.pack_operands(op, sc))
        FC.judge(op, sc, out, "device, %s; %s" % (FORMS[form], label))


@pytest.mark.gpu
def test_hip_fr_raw_ops_argument_checks(hz):
    c = hz.c
    one = np.zeros((5, 1, 9), dtype=np.uint32)
    out = np.zeros((1, 9), dtype=np.uint32)
    pin, pout = one.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    HZ_OK, HZ_ERR_ARG = 0, 1
    add = FC.OPS["fr_add"].code
    assert c.hz_fr_raw_ops(0, -1, 0, 1, pin, 1, pout) == HZ_ERR_ARG
    assert c.hz_fr_raw_ops(0, FC.N_OPS, 0, 1, pin, 1, pout) == HZ_ERR_ARG          # no such op
    assert c.hz_fr_raw_ops(0, add, 2, 1, pin, 2, pout) == HZ_ERR_ARG               # no such form
    assert c.hz_fr_raw_ops(0, add, -1, 1, pin, 2, pout) == HZ_ERR_ARG
    for op in FC.OPS.values():                                                      # an operand count that is not the op's
        for k in (len(op.kinds) - 1, len(op.kinds) + 1):
            assert c.hz_fr_raw_ops(0, op.code, 0, 1, pin, k, pout) == HZ_ERR_ARG, op.name
    assert c.hz_fr_raw_ops(0, add, 0, 1, None, 2, pout) == HZ_ERR_ARG              # null pointers
    assert c.hz_fr_raw_ops(0, add, 1, 1, pin, 2, None) == HZ_ERR_ARG
    assert b"hz_fr_raw_ops" in c.hz_last_error()
    for form in FORMS:                                                              # n = 0 is not an error, with or without buffers
        assert c.hz_fr_raw_ops(0, add, form, 0, None, 2, None) == HZ_OK
        assert hz.fr_raw_ops(add, form, np.zeros((2, 0, 9), dtype=np.uint32)).shape == (0, 9)
