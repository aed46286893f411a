"""What tests/test_capi_ledger_calls_cpu.py shares: the prototypes of the ledger's apply and verify calls and the members of their output
structs as include/hermez_witness.h states them, a stand-in for the loaded library that records every call and tags what it is handed, and
the one small batch every form is called with."""
import ctypes
import os
import re

import numpy as np

from circuits_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APPLY_CALLS = ("hz_ledger_apply_l2", "hz_ledger_apply_l2_signed", "hz_ledger_apply_l2_addr", "hz_ledger_apply_batch", "hz_ledger_apply_batch_exits",
               "hz_ledger_apply_batch_creates", "hz_ledger_apply_batch_atomic")
VERIFY_CALLS = ("hz_ledger_verify_l2", "hz_ledger_verify_l2_atomic")
DEV_CALLS = ("hz_ledger_outputs_dev", "hz_ledger_sig_outputs_dev", "hz_ledger_exit_outputs_dev", "hz_ledger_create_outputs_dev", "hz_ledger_withdraw_rows_dev")

# the members of the header's output structs, in the header's order (typed in from include/hermez_witness.h, not taken from capi's tuples)
_SIX = ("tokenID", "nonce", "sign", "balance", "ay", "ethAddr")
OUT_SLOTS = ([f + "1" for f in _SIX] + ["siblings1"] + [f + "2" for f in _SIX] + ["siblings2", "state_root_after", "acc_fee_after"] +
             [f + "3" for f in _SIX] + ["siblings3", "state_root_after_fee", "final_acc_fee", "old_root", "new_root"])            # hz_ledger_out
SIG_SLOTS = ["tx_compressed_data", "tx_compressed_data_v2", "sig_l2_hash"]                                                       # hz_ledger_sig_out
EXIT_SLOTS = ["new_exit", "is_old0_2", "old_key2", "old_value2", "exit_root_after", "new_exit_root"]                             # hz_ledger_exit_out
CREATE_SLOTS = ["aux_from_idx", "is_old0_1", "old_key1", "old_value1", "out_idx_after", "new_last_idx"]                          # hz_ledger_create_out
WITHDRAW_SLOTS = ["root_exit", "eth_addr", "token_id", "balance", "idx", "sign", "ay", "siblings_state", "status"]               # hz_withdraw_rows_out
STRUCT_ARGS = {"out": OUT_SLOTS, "sig_out": SIG_SLOTS, "exit_out": EXIT_SLOTS, "create_out": CREATE_SLOTS}
BYTE_ARGS = {"aux_to_idx_out": 0xA1, "l1_flags_out": 0xF1, "verdict_out": 0x07}
DEV_SLOTS = dict(zip(DEV_CALLS, (OUT_SLOTS, SIG_SLOTS, EXIT_SLOTS, CREATE_SLOTS, WITHDRAW_SLOTS)))
assert len(OUT_SLOTS) == 27


def prototype(fn):
    """the parameter names of `hz_status fn(...)` in the header, in order: the text between the parentheses without its comments, cut at
    the top-level commas, the last word of each piece"""
    text = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    args = re.search(r"hz_status %s\((.*?)\);" % fn, text, re.S).group(1)
    return [re.findall(r"\w+", piece)[-1] for piece in re.sub(r"/\*.*?\*/", "", args, flags=re.S).split(",")]


def value(a):
    """an argument as the integer C would see: None and a null c_void_p are 0"""
    return (a.value or 0) if isinstance(a, ctypes._SimpleCData) else (a or 0)


class Call:
    """one recorded call: args by the header's parameter names, as integers, and the bytes behind its input pointers at the time of the call"""

    def __init__(self, fn, args):
        self.fn, self.n_args = fn, len(args)
        self.args = dict(zip(prototype(fn), map(value, args)))
        a = self.args
        sizes = {"l1": (a.get("n_l1", 0), ctypes.sizeof(capi.hz_l1tx)), "from_bjj": (a.get("n_l1", 0), 32), "txs": (a["m"], ctypes.sizeof(capi.hz_l2tx)),
                 "sigs": (a["m"], ctypes.sizeof(capi.hz_l2sig)), "rq": (a["m"], ctypes.sizeof(capi.hz_l2rq)), "aux_to_idx": (a["m"], 8),
                 "fee_plan_tokens": (a.get("F", 0), 4), "fee_idxs": (a.get("F", 0), 8)}
        self.bytes = {name: ctypes.string_at(a[name], n * size) for name, (n, size) in sizes.items() if a.get(name)}


class Recorder:
    """stands where Lib.c stands. Every hz_ledger_apply_* / hz_ledger_verify_* records its call and writes through each output pointer that
    is not null: slot index + 1 into the first byte of every array a struct of pointers names, a byte of BYTE_ARGS through the plain ones.
    The *_dev getters fill their struct with DEV_BASE + 16 * slot."""
    DEV_BASE = 0x7000

    def __init__(self):
        self.calls = []
        for fn in APPLY_CALLS + VERIFY_CALLS:
            setattr(self, fn, lambda *args, fn=fn: self._apply(fn, args))
        for fn in DEV_CALLS:
            setattr(self, fn, lambda h, ptrs, fn=fn: self._dev(fn, ptrs))

    def hz_ledger_destroy(self, h):
        pass

    def _apply(self, fn, args):
        call = Call(fn, args)
        self.calls.append(call)
        for name, slots in STRUCT_ARGS.items():
            if call.args.get(name):
                for i, p in enumerate((ctypes.c_void_p * len(slots)).from_address(call.args[name])):
                    if p:
                        ctypes.c_uint8.from_address(p).value = i + 1
        for name, tag in BYTE_ARGS.items():
            if call.args.get(name):
                ctypes.c_uint8.from_address(call.args[name]).value = tag
        return 0

    def _dev(self, fn, ptrs):
        arr = (ctypes.c_void_p * len(DEV_SLOTS[fn])).from_address(value(ptrs))
        for i in range(len(arr)):
            arr[i] = self.DEV_BASE + 16 * i
        return 0


def ledgers(c, h=0xBEEF, k=4):
    """a Ledger and a GrowingLedger that were never created: made through __new__, their members set by hand, over the library stand-in c
    (or over a loaded Lib, given one) -> (dense, growing)"""
    if isinstance(c, capi.Lib):
        L = c
    else:
        L = capi.Lib.__new__(capi.Lib)
        L.c = c
    dense, growing = capi.Ledger.__new__(capi.Ledger), capi.GrowingLedger.__new__(capi.GrowingLedger)
    for led in (dense, growing):
        led.L, led.h, led.k, led.first_idx, led.device = L, h, k, 256, 0
    dense.N = 1 << k
    growing.capacity, growing.n_sib_max = 32, k
    return dense, growing


# the batch: n_l1 = 2 (the first row creates an account), m = 3 (the last an exit, linked to the row before it), F = 2
N_L1, M, F, N_SIB, K = 2, 3, 2, 5, 4
CHAIN_ID, NUM_BATCH = 0x1234, 0x77
L1_TXS = [{"fromIdx": 0, "toIdx": 0, "loadAmountF": 100, "tokenID": 1, "fromEthAddr": 0xA0A1, "fromBjjCompressed": (1 << 255) | 0xB0B1},
          {"fromIdx": 257, "toIdx": 258, "amountF": 3, "loadAmountF": 7, "tokenID": 1, "fromEthAddr": 0xA2A3}]
TXS = [{"fromIdx": 256, "toIdx": 257, "amountF": 5, "nonce": 0, "tokenID": 1, "userFee": 10, "s": 11, "r8x": 12, "r8y": 13, "maxNumBatch": 200},
       {"fromIdx": 257, "toIdx": 0, "amountF": 6, "nonce": 1, "tokenID": 2, "userFee": 20, "s": 21, "r8x": 22, "r8y": 23, "toEthAddr": 0xE0E1, "toBjjAy": 0xB2,
        "toBjjSign": 1},
       {"fromIdx": 258, "toIdx": 1, "amountF": 9, "nonce": 2, "tokenID": 1, "userFee": 30, "s": 31, "r8x": 32, "r8y": 33, "rqOffset": 7, "rqTxCompressedDataV2": 0xC0C1,
        "rqToEthAddr": 0xE0E1, "rqToBjjAy": 0xB2}]
PLAN, IDXS, AUX = [1, 2], [256, 259], [0, 300, 0]


def inputs(n_l1=N_L1, m=M):
    """the expected bytes behind every input pointer, from arrays built directly"""
    return {"l1": bytes(capi.l1tx_array(L1_TXS[:n_l1]))[:n_l1 * ctypes.sizeof(capi.hz_l1tx)], "from_bjj": capi.from_bjj_array(L1_TXS)[:n_l1].tobytes(),
            "txs": bytes(capi.l2tx_array(TXS[:m]))[:m * ctypes.sizeof(capi.hz_l2tx)], "sigs": bytes(capi.l2sig_array(TXS[:m]))[:m * ctypes.sizeof(capi.hz_l2sig)],
            "rq": bytes(capi.l2rq_array(TXS))[:m * ctypes.sizeof(capi.hz_l2rq)], "aux_to_idx": np.array(AUX[:m], dtype=np.uint64).tobytes(),
            "fee_plan_tokens": np.array(PLAN, dtype=np.uint32).tobytes(), "fee_idxs": np.array(IDXS, dtype=np.uint64).tobytes()}


def shapes(form, n_l1=N_L1, m=M, n_sib=N_SIB, verify=True):
    """{name: shape} of what apply form `form` (the C function's name) returns, in order"""
    batch = form not in APPLY_CALLS[:3]
    R = (n_l1 if batch else 0) + m
    rows, sib = {"1": R, "2": R, "3": F}, min(max(n_sib, 0), 64)
    out = {}
    for name in OUT_SLOTS:
        r = rows.get(name[-1], {"state_root_after": R, "acc_fee_after": R, "state_root_after_fee": F, "final_acc_fee": F, "old_root": 1, "new_root": 1}.get(name))
        out[name] = (r, sib, 32) if name.startswith("siblings") else (r, F, 32) if name == "acc_fee_after" else (r, 32)
    if form == "hz_ledger_apply_l2_signed" or (verify and form != "hz_ledger_apply_l2"):
        out.update({name: (m, 32) for name in SIG_SLOTS})
    if form not in APPLY_CALLS[:2]:
        out["auxToIdx"] = (R, 32)
    if batch:
        out["l1_flags"] = (n_l1,)
        if form != "hz_ledger_apply_batch":
            out.update({name: (R, 32) for name in EXIT_SLOTS[:-1]}, new_exit_root=(1, 32))
        if form in APPLY_CALLS[5:]:
            out.update({name: (R, 32) for name in CREATE_SLOTS[:-1]}, new_last_idx=(1, 32))
    return out


def tags():
    """{name: the byte the stand-in writes into the array's first place}"""
    t = {name: i + 1 for slots in STRUCT_ARGS.values() for i, name in enumerate(slots)}
    t.update(auxToIdx=BYTE_ARGS["aux_to_idx_out"], l1_flags=BYTE_ARGS["l1_flags_out"])
    return t
