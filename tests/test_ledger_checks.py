"""The argument checks of the ledger's device calls (csrc/ledger_checks.h, in the order ledger_prepare, ledger_verify and
hz_ledger_select_batch run them) on the gpu part of tests/golden/ledger_arg_errors.json.gz: every apply form, both verify forms and
hz_ledger_select_batch on a dense ledger of k = 4, a growing one of capacity 16, ledgers that hold nothing and a null one -- one failing
check of each kind and the pairs that fix the order in which errors win, recorded on the commit before the checks moved. Every case ends in
the host's checks (reason 9, a destination nobody holds, behind the lookup): nothing is applied."""
import pytest

import ledger_arg_errors_common as E

pytestmark = pytest.mark.gpu


def test_the_device_calls_answer_as_recorded(hz):
    cases = E.load("gpu")
    assert {c["call"] for c in cases} == set(E.APPLY + E.VERIFY + (E.SELECT,)) and {c["ledger"] for c in cases} == set(E.LEDGERS)
    assert all(c["status"] for c in cases) and len({c["message"] for c in cases}) >= 400
    ledgers, close = E.open_ledgers(hz)
    sizes = {name: hz.c.hz_ledger_size(h) for name, h in ledgers.items() if h}
    wrong = [(c["call"], c["ledger"], c["args"], got, (c["status"], c["message"])) for c in cases for got in [E.call(hz, c, ledgers)] if got != (c["status"], c["message"])]
    assert sizes == {name: hz.c.hz_ledger_size(h) for name, h in ledgers.items() if h}    # no case created an account
    close()
    assert not wrong, wrong[:5]
