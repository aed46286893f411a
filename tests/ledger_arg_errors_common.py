"""The argument errors of the ledger's calls as recorded cases (tests/golden/ledger_arg_errors.json.gz, a JSON list): what a case holds, how it is put to
the library, and how it reads in the line format of tests/native/ledger_checks_check.cpp.

A case is {"part": "cpu" | "gpu", "call", "args", "status", "message"}; the gpu part also names its "ledger" (LEDGERS). args:
  rows      l1 [[from_idx, to_idx, amount_f, load_amount_f, token_id, from_eth_addr]], txs [[from_idx, to_idx, amount_f, nonce, token_id,
            user_fee]], sigs [[s, r8x, r8y, to_eth_addr, to_bjj_ay, max_num_batch, to_bjj_sign]], rq [[v2, to_eth_addr, to_bjj_ay, offset]];
            256-bit values are hexadecimal strings. txs_times: the txs rows repeated
  vectors   toks, idxs, aux, partner, kept, from_bjj (hexadecimal strings, one per L1 row)
  counts    n_l1, m, F: the length of l1, txs, toks where they are not stated
  numbers   k, first_idx, n_sib, growing, capacity, size, flags, chain_id, max_keep
  pointers  an array that is missing or null is a null pointer; sig_out / out: true for a structure of null members
Every array goes to C in a buffer of exactly its size. `python tests/ledger_arg_errors_common.py cpu|gpu FILE` records cpu_cases() or gpu_cases()
with the library that is loaded, `... join FILE FILE` makes the golden file of the two: the golden file is made on the commit BEFORE a change of the checks, never on the one under test."""
import ctypes
import gzip
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from circuits_amd import capi  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ledger_arg_errors.json.gz")
FIRST = 256
P = capi.R_MODULUS
NUM_BATCH = 7
# the ledgers of the gpu part: a dense one of k = 4, a growing one of capacity 16 holding four accounts, and one of each that holds nothing
LEDGERS = ("dense", "growing", "dense empty", "growing unloaded", "null")
K, CAPACITY, LIVE, N_SIB_MAX = 4, 16, 4, 33


def _int(v):
    return int(v, 16) if isinstance(v, str) else int(v)


def _b32(v):
    return (ctypes.c_uint8 * 32)(*_int(v).to_bytes(32, "little"))


def _l1(rows):
    arr = (capi.hz_l1tx * len(rows))()
    for g, r in zip(arr, rows):
        g.from_idx, g.to_idx, g.amount_f, g.load_amount_f, g.token_id, g.from_eth_addr = r[0], r[1], r[2], r[3], r[4], _b32(r[5])
    return arr


def _txs(rows):
    arr = (capi.hz_l2tx * len(rows))()
    for i, r in enumerate(rows):
        arr[i] = capi.hz_l2tx(*r)
    return arr


def _sigs(rows):
    arr = (capi.hz_l2sig * len(rows))()
    for g, r in zip(arr, rows):
        g.s, g.r8x, g.r8y, g.to_eth_addr, g.to_bjj_ay, g.max_num_batch, g.to_bjj_sign = _b32(r[0]), _b32(r[1]), _b32(r[2]), _b32(r[3]), _b32(r[4]), r[5], r[6]
    return arr


def _rq(rows):
    arr = (capi.hz_l2rq * len(rows))()
    for g, r in zip(arr, rows):
        g.rq_tx_compressed_data_v2, g.rq_to_eth_addr, g.rq_to_bjj_ay, g.rq_offset = _b32(r[0]), _b32(r[1]), _b32(r[2]), r[3]
    return arr


def _vec(ctype):
    return lambda vals: (ctype * len(vals))(*vals)


def _keys(vals):
    return (ctypes.c_uint8 * (32 * len(vals)))(*b"".join(_int(v).to_bytes(32, "little") for v in vals))


ARRAYS = {"l1": _l1, "txs": _txs, "sigs": _sigs, "rq": _rq, "toks": _vec(ctypes.c_uint32), "idxs": _vec(ctypes.c_uint64), "aux": _vec(ctypes.c_uint64),
          "partner": _vec(ctypes.c_int32), "kept": _vec(ctypes.c_uint8), "from_bjj": _keys}
NUMBERS = {"k": K, "first_idx": FIRST, "n_sib": K, "growing": 1, "capacity": CAPACITY, "size": LIVE, "flags": 0, "chain_id": 1, "max_keep": 4096}


def marshal(args):
    """-> (the numbers and counts, {array name: its buffer, None for a null pointer})"""
    a = dict(args)
    if a.get("txs") is not None:
        a["txs"] = a["txs"] * a.pop("txs_times", 1)
    bufs = {name: make(a[name]) if a.get(name) is not None else None for name, make in ARRAYS.items()}
    num = {name: a.get(name, default) for name, default in NUMBERS.items()}
    for count, of in (("n_l1", "l1"), ("m", "txs"), ("F", "toks")):
        num[count] = a[count] if count in a else len(a[of]) if a.get(of) is not None else 0
    return num, bufs


def lines(case):
    """the case for tests/native/ledger_checks_check.cpp: its call, the numbers, every array as the bytes C is given"""
    num, bufs = marshal(case["args"])
    out = ["case " + case["call"]] + ["n %s %x" % (name, v) for name, v in sorted(num.items())]
    out += ["a %s %s" % (name, "null" if b is None else "%x %s" % (len(bytes(b)), bytes(b).hex() or "-")) for name, b in sorted(bufs.items())]
    return out + ["end"]


def expected_line(case):
    return "%d\t%s" % (case["status"], case["message"])


def _null_members(n):
    return (ctypes.c_void_p * n)()


def call(L, case, ledgers=None):
    """the case put to the loaded library -> (status, message: hz_last_error's text of a failure, "" of a success)"""
    num, b = marshal(case["args"])
    keep = []

    def p(name):
        return None if b[name] is None else ctypes.addressof(b[name])

    def flag(name, members):    # an output structure: null, or one of null members
        if not case["args"].get(name):
            return None
        keep.append(_null_members(members))
        return ctypes.addressof(keep[-1])
    fn = case["call"]
    n_l1, m, F, first = num["n_l1"], num["m"], num["F"], num["first_idx"]
    fees = (F, p("toks"), p("idxs"))
    if fn == "hz_ledger_plan_l2":
        argv = (m, p("txs")) + fees + (num["k"], first) + (None,) * 7
    elif fn == "hz_ledger_plan_batch":
        argv = (n_l1, p("l1"), m, p("txs")) + fees + (num["k"], first) + (None,) * 11
    elif fn == "hz_ledger_plan_exits":
        argv = (n_l1, p("l1"), m, p("txs")) + fees + (num["k"], first, num["n_sib"]) + (None,) * 15
    elif fn == "hz_ledger_plan_creates":
        argv = (n_l1, p("l1"), p("from_bjj"), m, p("txs")) + fees + (num["growing"], num["capacity"], first, num["size"]) + (None,) * 3
    elif fn == "hz_ledger_plan_atomic":
        argv = (n_l1, m, p("txs"), p("sigs"), p("rq"), None, None)
    elif fn == "hz_ledger_plan_select":
        argv = (n_l1, p("l1"), m, p("txs"), p("aux"), p("partner"), p("kept")) + (None,) * 6
    elif fn == "hz_ledger_plan_main_inputs":
        some = ctypes.addressof(_keep(keep, ctypes.c_uint64 * 1))
        given = [None if name in case["args"].get("null", ()) else some for name in ("names", "offsets", "widths", "flat_lens")]
        argv = (0,) + tuple(given) + (0, 4, 16, 2, 2, 0) + (None,) * 4
    else:
        led = ledgers[case["ledger"]]
        tail = (num["flags"], p("aux"), num["chain_id"], NUM_BATCH) + fees + (num["n_sib"], None, flag("sig_out", 3), None)
        batch = (led, n_l1, p("l1"))
        if fn == "hz_ledger_apply_l2":
            argv = (led, m, p("txs")) + fees + (num["n_sib"], None)
        elif fn == "hz_ledger_apply_l2_signed":
            argv = (led, m, p("txs"), p("sigs"), num["chain_id"], NUM_BATCH) + fees + (num["n_sib"], None, flag("sig_out", 3))
        elif fn in ("hz_ledger_verify_l2", "hz_ledger_verify_l2_atomic"):
            verdict = None if case["args"].get("verdict_out") is False else ctypes.addressof(_keep(keep, ctypes.c_uint8 * max(m, 1)))
            argv = (led, m, p("txs"), p("sigs")) + ((p("rq"),) if fn.endswith("atomic") else ()) + (num["chain_id"], NUM_BATCH, verdict, None)
        elif fn == "hz_ledger_apply_l2_addr":
            argv = (led, m, p("txs"), p("sigs")) + tail
        elif fn == "hz_ledger_apply_batch":
            argv = batch + (m, p("txs"), p("sigs")) + tail + (None,)
        elif fn == "hz_ledger_apply_batch_exits":
            argv = batch + (m, p("txs"), p("sigs")) + tail + (None, None)
        elif fn == "hz_ledger_apply_batch_creates":
            argv = batch + (p("from_bjj"), m, p("txs"), p("sigs")) + tail + (None, None, None)
        elif fn == "hz_ledger_apply_batch_atomic":
            argv = batch + (p("from_bjj"), m, p("txs"), p("sigs"), p("rq")) + tail + (None, None, None)
        elif fn == "hz_ledger_select_batch":
            out = None if case["args"].get("out") is False else ctypes.addressof(_keep(keep, ctypes.c_void_p * 6))
            argv = batch + (p("from_bjj"), m, p("txs"), p("sigs"), p("rq"), p("partner"), num["flags"], num["chain_id"], NUM_BATCH, num["max_keep"], out)
        else:
            raise KeyError(fn)
    st = getattr(L.c, fn)(*argv)
    return st, L.c.hz_last_error().decode() if st else ""


def _keep(keep, ctype):
    keep.append(ctype())
    return keep[-1]


def open_ledgers(L):
    """the ledgers of the gpu part as handles -> ({name: handle}, close)"""
    import numpy as np

    def cols(n):    # token 1, nonce 0; a balance; a key and an address of its own
        e0, bal, ay, eth = (np.zeros((n, 32), dtype=np.uint8) for _ in range(4))
        e0[:, 0] = 1
        bal[:, 2] = 1
        ay[:, 0] = np.arange(n) + 1
        eth[:, 0] = np.arange(n) + 1
        eth[:, 1] = 0x10
        return [a.ctypes.data for a in (e0, bal, ay, eth)], (e0, bal, ay, eth)
    h = {name: ctypes.c_void_p() for name in LEDGERS[:4]}
    L._check(L.c.hz_ledger_create(0, K, FIRST, ctypes.byref(h["dense"])))
    L._check(L.c.hz_ledger_create(0, K, FIRST, ctypes.byref(h["dense empty"])))
    L._check(L.c.hz_ledger_create_growing(0, CAPACITY, FIRST, N_SIB_MAX, ctypes.byref(h["growing"])))
    L._check(L.c.hz_ledger_create_growing(0, CAPACITY, FIRST, N_SIB_MAX, ctypes.byref(h["growing unloaded"])))
    ptrs, held = cols(1 << K)
    L._check(L.c.hz_ledger_load(h["dense"], *ptrs))
    ptrs, held = cols(LIVE)    # (held: the arrays behind the pointers, alive until the call returns)
    L._check(L.c.hz_ledger_load_accounts(h["growing"], LIVE, *ptrs))
    handles = dict(h, null=None)

    def close():
        for v in h.values():
            L.c.hz_ledger_destroy(v)
    return handles, close


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
LAST = FIRST + (1 << K) - 1
ABOVE_R = "%x" % (P + 5)
ETH = "1001"           # the address of account FIRST in the gpu part's ledgers
NOBODY = "77777777"    # an address no account holds


def tx(frm, to, amount_f=5, nonce=0, token=1, fee=0):
    return [frm, to, amount_f, nonce, token, fee]


def l1(frm, to=0, amount_f=0, load=9, token=1, eth="1234"):
    return [frm, to, amount_f, load, token, eth]


def sig(s="1", r8x="2", r8y="3", eth="0", ay="0", mnb=0, sign=0):
    return [s, r8x, r8y, eth, ay, mnb, sign]


def rq(v2="0", eth="0", ay="0", off=0):
    return [v2, eth, ay, off]


GARBAGE_NOP = [0, 1 << 50, 1 << 60, 9, 3, 200]    # from_idx == 0: the row is not looked at
T_OK, T_OK2 = tx(FIRST, FIRST + 1), tx(FIRST + 1, FIRST + 2)
BAD_FROM, BAD_TO, BAD_AMOUNT = tx(LAST + 1, FIRST), tx(FIRST, LAST + 1), tx(FIRST, FIRST + 1, 1 << 40)
FEE = {"toks": [1], "idxs": [FIRST + 3]}
BAD_FEE = {"toks": [1], "idxs": [LAST + 1]}


def _l2_row_cases(call, base, exits, by_addr):
    """the per-row checks of ledger_check_txs as `call` has them; base: the other arguments"""
    out = [dict(base, txs=[tx(FIRST, LAST)]), dict(base, txs=[tx(LAST, FIRST)]), dict(base, txs=[T_OK, BAD_FROM]), dict(base, txs=[T_OK, tx(FIRST - 1, FIRST)]),
           dict(base, txs=[BAD_TO]), dict(base, txs=[T_OK, BAD_AMOUNT]), dict(base, txs=[GARBAGE_NOP, T_OK]), dict(base, txs=[tx(FIRST, 0)]), dict(base, txs=[tx(FIRST, 1)]),
           dict(base, txs=[tx(FIRST, 0, 1 << 40)]), dict(base, txs=[tx(FIRST, 1, 1 << 40)]), dict(base, txs=[BAD_FROM, BAD_AMOUNT])]
    return [(call, a) for a in out]


def _l1_row_cases(call, base, last=LAST):
    out = [dict(base, l1=[l1(FIRST, last, 3)]), dict(base, l1=[l1(last, FIRST, 3)]), dict(base, l1=[l1(FIRST), l1(last + 1)]), dict(base, l1=[l1(FIRST, last + 1, 3)]),
           dict(base, l1=[l1(FIRST, 1, 3)]), dict(base, l1=[l1(0, 0)]), dict(base, l1=[l1(FIRST, FIRST, 1 << 40)]), dict(base, l1=[l1(FIRST, 0, 0, 1 << 40)]),
           dict(base, l1=[l1(FIRST, 0, 0, 9, 1, "1" + "0" * 40)]), dict(base, l1=[l1(FIRST, 0, 0, 9, 1, "ff" * 20)]), dict(base, l1=[l1(FIRST, 0, 3)]),
           dict(base, l1=[l1(FIRST, 0, 1 << 35)]), dict(base, n_l1=513, l1=[l1(FIRST)]), dict(base, n_l1=1), dict(base, n_l1=0),
           dict(base, l1=[l1(LAST + 1, 0, 1 << 40)]), dict(base, l1=[l1(FIRST, 0, 3, 1 << 40, 1, "1" + "0" * 40)])]
    return [(call, a) for a in out]


def _plan_cases(call, base, exits, by_addr):
    """ledger_check_plan's own checks"""
    out = [dict(base, m=1), dict(base, F=1, toks=[1]), dict(base, F=1, idxs=[FIRST]), dict(base, m=0, F=0), dict(base, toks=[1] * 65, idxs=[0] * 65),
           dict(base, toks=[1] * 64, idxs=[0] * 64), dict(base, m=(1 << 20) + 1, txs=[T_OK]), dict(base, txs=[T_OK], **BAD_FEE), dict(base, txs=[T_OK], toks=[1, 2], idxs=[0, LAST]),
           dict(base, txs=[T_OK], toks=[1, 2], idxs=[FIRST, FIRST - 1]),
           dict(base, txs=[BAD_FROM], **BAD_FEE), dict(base, m=1, toks=[1] * 65, idxs=[0] * 65), dict(base, m=(1 << 20) + 1, txs=[T_OK], toks=[1] * 65, idxs=[0] * 65)]
    if call == "hz_ledger_plan_l2":    # 65538 and 65536 updates
        out += [dict(base, txs=[T_OK], txs_times=32769), dict(base, txs=[T_OK], txs_times=32768)]
    return [(call, a) for a in out]


def cpu_cases():
    c = []
    for call, base, exits in (("hz_ledger_plan_l2", {}, False), ("hz_ledger_plan_batch", {}, False), ("hz_ledger_plan_exits", {}, True),
                              ("hz_ledger_plan_creates", {"size": 1 << K, "capacity": 1 << K}, True)):
        creates = call.endswith("creates")
        c += _plan_cases(call, base, exits, call != "hz_ledger_plan_l2") + _l2_row_cases(call, base, exits, call != "hz_ledger_plan_l2")
        if not creates:
            c += [(call, dict(base, k=3)), (call, dict(base, k=25)), (call, dict(base, k=24, first_idx=2, txs=[tx((1 << 24) + 1, 2)])), (call, dict(base, k=3, txs=[BAD_FROM]))]
        if call != "hz_ledger_plan_l2":
            c += _l1_row_cases(call, base) + [(call, dict(base, l1=[l1(LAST + 1)], txs=[BAD_FROM]))]
        if call == "hz_ledger_plan_batch":    # the L1 run's updates count
            c += [(call, dict(base, l1=[l1(FIRST, FIRST + 1, 3)] * 512, txs=[T_OK], txs_times=32257)), (call, dict(base, l1=[l1(FIRST, FIRST + 1, 3)] * 512, txs=[T_OK], txs_times=32256))]
    x = "hz_ledger_plan_exits"
    c += [(x, {"n_sib": 3}), (x, {"n_sib": 65}), (x, {"n_sib": 64, "txs": [tx(FIRST, 1)]}), (x, {"k": 3, "n_sib": 2}), (x, {"n_sib": 3, "l1": [l1(0)]}),
          (x, {"n_sib": 4, "txs": [tx(FIRST, 1), tx(FIRST + 16, 1)], "first_idx": FIRST}), (x, {"n_sib": 4, "l1": [l1(FIRST, 1, 3), l1(FIRST + 1, 1, 3), l1(FIRST + 2, 1, 3)]}),
          (x, {"n_sib": 4, "txs": [tx(FIRST, 1), tx(FIRST + 8, 1)]}), (x, {"n_sib": 5, "txs": [tx(FIRST, 1), tx(FIRST + 8, 1)]}),
          (x, {"n_sib": 4, "l1": [l1(FIRST + 1, 1, 3)], "txs": [T_OK, tx(FIRST + 9, 1)]})]
    k = "hz_ledger_plan_creates"
    key = ["5"]
    c += [(k, {"capacity": 0}), (k, {"capacity": (1 << 24) + 1}), (k, {"size": 17}), (k, {"first_idx": 1}), (k, {"capacity": 1 << 24, "size": 1 << 24, "first_idx": 2}),
          (k, {"growing": 0, "l1": [l1(0)], "from_bjj": key}), (k, {"l1": [l1(0)]}), (k, {"size": 16, "l1": [l1(0)], "from_bjj": key}),
          (k, {"size": 15, "l1": [l1(0), l1(0)], "from_bjj": key * 2}), (k, {"size": 15, "l1": [l1(0)], "from_bjj": key}), (k, {"l1": [l1(0, 1, 3)], "from_bjj": key}),
          (k, {"l1": [l1(0, FIRST + LIVE, 3)], "from_bjj": key}), (k, {"l1": [l1(0, FIRST + LIVE + 1, 3)], "from_bjj": key}), (k, {"l1": [l1(FIRST + LIVE)]}),
          (k, {"l1": [l1(0), l1(FIRST + LIVE)], "from_bjj": key * 2}), (k, {"size": 0, "l1": [l1(FIRST)]}), (k, {"size": 0, "l1": [l1(0), l1(FIRST, FIRST, 3)], "from_bjj": key * 2}),
          (k, {"size": 0, "l1": [l1(0, FIRST, 3)], "from_bjj": key}), (k, {"l1": [l1(0)], "from_bjj": key, "txs": [tx(FIRST + LIVE, FIRST)]}),
          (k, {"l1": [l1(0)], "from_bjj": key, "txs": [tx(FIRST + LIVE + 1, FIRST)]}), (k, {"l1": [l1(0)], "from_bjj": key, "toks": [1], "idxs": [FIRST + LIVE + 1]}),
          (k, {"l1": [l1(0, 0, 1 << 40)], "growing": 0}), (k, {"l1": [l1(FIRST, 1, 3)]}), (k, {"l1": [l1(FIRST + 1, FIRST, 1 << 40)]}),
          (k, {"l1": [l1(FIRST + LIVE, FIRST + LIVE + 1, 3)]}), (k, {"l1": [l1(0, 0, 0, 1 << 40)], "from_bjj": key})]
    a = "hz_ledger_plan_atomic"
    two = {"txs": [T_OK, T_OK2], "sigs": [sig(), sig()]}
    c += [(a, {}), (a, {"m": 1, "sigs": [sig()]}), (a, {"m": 1, "txs": [T_OK]}), (a, {"n_l1": 513}), (a, {"n_l1": 512}), (a, dict(two, m=(1 << 20) + 1)),
          (a, dict(two, n_l1=513, m=(1 << 20) + 1)), (a, two), (a, dict(two, rq=[rq(), rq(off=8)])), (a, dict(two, rq=[rq(), rq(off=7)])), (a, dict(two, rq=[rq(v2=ABOVE_R), rq()])),
          (a, dict(two, rq=[rq(eth=ABOVE_R), rq()])), (a, dict(two, rq=[rq(), rq(ay=ABOVE_R)])), (a, dict(two, rq=[rq(v2="%x" % (P - 1)), rq()])),
          (a, dict(two, rq=[rq(off=9, v2=ABOVE_R), rq()])), (a, {"txs": [GARBAGE_NOP, T_OK], "sigs": [sig(), sig()], "rq": [rq(off=200, ay=ABOVE_R), rq()]}),
          (a, dict(two, n_l1=513, rq=[rq(off=8), rq()]))]
    s = "hz_ledger_plan_select"
    pool = {"txs": [T_OK, T_OK2, tx(FIRST + 2, 0)]}
    c += [(s, {}), (s, {"n_l1": 1}), (s, {"m": 1}), (s, {"n_l1": 513, "l1": [l1(FIRST)]}), (s, {"l1": [l1(0)]}), (s, {"l1": [l1(FIRST, 0, 3)]}), (s, {"l1": [l1(FIRST, 5, 1 << 40)]}),
          (s, {"m": 4097, "txs": [T_OK]}), (s, {"txs": [T_OK], "txs_times": 4096}), (s, pool), (s, dict(pool, partner=[1, 0, -1])), (s, dict(pool, partner=[3, 0, -1])),
          (s, dict(pool, partner=[2, 0, -1])), (s, dict(pool, partner=[-2, 0, -1])), (s, dict(pool, partner=[-1, 1, -1])), (s, dict(pool, partner=[0, -1, -1])),
          (s, {"txs": [GARBAGE_NOP, T_OK], "partner": [77, -1]}), (s, dict(pool, aux=[0, 0, FIRST + 9], kept=[1, 1, 1], partner=[1, 0, -1])),
          (s, {"l1": [l1(0)], "m": 4097, "txs": [T_OK]}), (s, {"m": 4097, "txs": [T_OK], "partner": [5]}), (s, {"txs": [tx(FIRST + i, FIRST + 5000 + i) for i in range(2049)]}),
          (s, {"txs": [tx(FIRST + i, FIRST + 5000 + i) for i in range(2048)]}), (s, {"l1": [l1(FIRST, 0, 0, 1 << 40)], "m": 1})]
    mi = "hz_ledger_plan_main_inputs"
    c += [(mi, {"null": [name]}) for name in ("names", "offsets", "widths", "flat_lens")] + [(mi, {})]
    return [{"part": "cpu", "call": call, "args": args} for call, args in c]


APPLY = ("hz_ledger_apply_l2", "hz_ledger_apply_l2_signed", "hz_ledger_apply_l2_addr", "hz_ledger_apply_batch", "hz_ledger_apply_batch_exits", "hz_ledger_apply_batch_creates",
         "hz_ledger_apply_batch_atomic")
VERIFY = ("hz_ledger_verify_l2", "hz_ledger_verify_l2_atomic")
SELECT = "hz_ledger_select_batch"


def gpu_cases():
    c = []
    one = {"txs": [T_OK], "sigs": [sig()]}
    bad_s = {"txs": [T_OK], "sigs": [sig(s=ABOVE_R)]}
    to_nobody = {"txs": [tx(FIRST, 0)], "sigs": [sig(eth=NOBODY)]}
    for call in APPLY + VERIFY + (SELECT,):
        apply, plain, batch = call in APPLY, call in APPLY[:2], call in APPLY[3:] or call == SELECT
        takes_creates, takes_exits, takes_rq = call in APPLY[5:] or call == SELECT, call in APPLY[4:] or call == SELECT, "atomic" in call or call == SELECT
        signed = call != "hz_ledger_apply_l2"
        verify = {"flags": 1} if not plain and call not in VERIFY else {}
        for led in ("null", "dense empty", "growing unloaded"):
            c.append((call, led, one))
        for led in ("dense", "growing"):
            last = LAST if led == "dense" else FIRST + LIVE - 1
            n_sib = {"n_sib": K if led == "dense" else 8}
            ok, ok_s = dict(one, **n_sib), dict(one, **n_sib, **verify)
            c += [(call, led, dict(ok, txs=[tx(last + 1, FIRST)])), (call, led, dict(ok, txs=[tx(FIRST, last + 1)])), (call, led, dict(ok, txs=[tx(FIRST, last, 1 << 40)])),
                  (call, led, dict(ok, m=1, txs=None)), (call, led, dict(ok, m=(1 << 20) + 1))]
            if plain or call in VERIFY:
                c.append((call, led, dict(ok, txs=[tx(FIRST, 0)])))
            if not takes_exits:
                c.append((call, led, dict(ok, txs=[tx(FIRST, 1)])))
            if apply:
                c += [(call, led, dict(one, n_sib=K - 1 if led == "dense" else 0)), (call, led, dict(one, n_sib=65)), (call, led, dict(one, n_sib=N_SIB_MAX + 1 if led == "growing" else 0)),
                      (call, led, dict(ok, toks=[1] * 65, idxs=[0] * 65)), (call, led, dict(ok, **BAD_FEE) if led == "dense" else dict(ok, toks=[1], idxs=[last + 1])),
                      (call, led, dict(ok, F=1)), (call, led, dict(one, n_sib=65, txs=[BAD_FROM])), (call, led, dict(ok_s, toks=[1], idxs=[LAST + 1], sigs=[sig(s=ABOVE_R)]))]
            if signed:
                c += [(call, led, dict(ok_s, sigs=None)), (call, led, dict(ok_s, chain_id=1 << 16)), (call, led, dict(ok_s, sigs=[sig(sign=2)])),
                      (call, led, dict(ok_s, sigs=[sig(eth="1" + "0" * 40)])), (call, led, dict(ok_s, **bad_s)), (call, led, dict(ok_s, sigs=[sig(r8x=ABOVE_R)])),
                      (call, led, dict(ok_s, sigs=[sig(r8y=ABOVE_R)])), (call, led, dict(ok_s, sigs=[sig(ay=ABOVE_R)])), (call, led, dict(ok_s, txs=[BAD_TO], sigs=[sig(s=ABOVE_R)])),
                      (call, led, dict(ok_s, txs=[GARBAGE_NOP, tx(FIRST, last + 1)], sigs=[sig(s=ABOVE_R, sign=9), sig()]))]
            if verify:    # the forms with flags
                c += [(call, led, dict(ok, flags=2)), (call, led, dict(ok, flags=3, n_sib=65)), (call, led, dict(ok, sigs=[sig(s=ABOVE_R, ay=ABOVE_R)], chain_id=1 << 16)),
                      (call, led, dict(ok, sigs=None, txs=[tx(FIRST, 0)]))]
                if not batch:
                    c.append((call, led, dict(ok, sigs=None)))
                if apply:
                    c += [(call, led, dict(ok, **to_nobody)), (call, led, dict(ok, sig_out=True)), (call, led, dict(ok, sig_out=True, n_sib=65)), (call, led, dict(ok, txs=[tx(FIRST, 0)], sigs=[sig(eth=ETH)], aux=[last + 1])),
                          (call, led, dict(ok, txs=[tx(FIRST, 0)], sigs=[sig(eth=ETH)], aux=[0])), (call, led, dict(ok, txs=[T_OK, tx(FIRST, 0)], sigs=[sig(), sig(eth=NOBODY)], **FEE))]
            if batch:
                b = dict(ok, from_bjj=None)
                c += [(call, led, dict(b, l1=[l1(last + 1)])), (call, led, dict(b, l1=[l1(FIRST, last + 1, 3)])), (call, led, dict(b, l1=[l1(0)])),
                      (call, led, dict(b, n_l1=513, l1=[l1(FIRST)])), (call, led, dict(b, n_l1=1)), (call, led, dict(b, l1=[l1(FIRST, 0, 1 << 40)])),
                      (call, led, dict(b, l1=[l1(FIRST, 0, 0, 1 << 40)])), (call, led, dict(b, l1=[l1(FIRST, 0, 0, 9, 1, "1" + "0" * 40)])), (call, led, dict(b, l1=[l1(FIRST, 0, 3)])),
                      (call, led, dict(b, l1=[l1(last + 1)], txs=[BAD_FROM]))]
                if not takes_exits:
                    c.append((call, led, dict(b, l1=[l1(FIRST, 1, 3)])))
                if apply:
                    c.append((call, led, dict(b, l1=[l1(FIRST)], n_sib=65)))
                if takes_creates:
                    key = ["5"]
                    c += [(call, led, dict(b, l1=[l1(0), l1(0, 1)], from_bjj=key * 2)), (call, led, dict(b, l1=[l1(0, 1, 3)], from_bjj=key)), (call, led, dict(b, l1=[l1(0)] * 13, from_bjj=key * 13)),
                          (call, led, dict(b, l1=[l1(0), l1(last + 2)], from_bjj=key * 2)), (call, led, dict(b, l1=[l1(0, last + 2, 3)], from_bjj=key)),
                          (call, led, dict(b, l1=[l1(0)], from_bjj=key, txs=[tx(last + 2, FIRST)]))]
            if takes_rq:
                r = dict(ok, txs=[T_OK, T_OK2], sigs=[sig(), sig()])
                if call != SELECT:    # (the selection makes the offsets itself)
                    c.append((call, led, dict(r, rq=[rq(), rq(off=8)])))
                c += [(call, led, dict(r, rq=[rq(v2=ABOVE_R), rq()])), (call, led, dict(r, rq=[rq(), rq(eth=ABOVE_R)])),
                      (call, led, dict(r, rq=[rq(), rq(ay=ABOVE_R)])), (call, led, dict(r, rq=[rq(ay=ABOVE_R), rq()], sigs=[sig(), sig(ay=ABOVE_R)])),
                      (call, led, dict(r, txs=[T_OK, tx(FIRST, 0)], sigs=[sig(), sig(eth=NOBODY)], rq=[rq(eth=ABOVE_R), rq()]))]
            if call in VERIFY:
                c += [(call, led, dict(ok, verdict_out=False)), (call, led, dict(ok, verdict_out=False, txs=None, m=1))]
            if call == SELECT:
                p = dict(ok, txs=[T_OK, T_OK2], sigs=[sig(), sig()])
                c += [(call, led, dict(ok, out=False)), (call, led, dict(ok, m=4097)), (call, led, dict(p, partner=[2, -1])), (call, led, dict(p, partner=[0, -1])),
                      (call, led, dict(p, partner=[-5, 0])), (call, led, dict(p, partner=[1, 0], rq=[rq(off=200), rq(v2=ABOVE_R)])), (call, led, dict(p, partner=[2, -1], sigs=None)),
                      (call, led, dict(ok, m=4097, l1=[l1(last + 1)])), (call, led, dict(ok, out=False, flags=2))]
    return [{"part": "gpu", "call": call, "ledger": led, "args": args} for call, led, args in c]


def record(part, path):
    L = capi.lib()
    cases = {"cpu": cpu_cases, "gpu": gpu_cases}[part]()
    ledgers, close = open_ledgers(L) if part == "gpu" else (None, lambda: None)
    for case in cases:
        case["status"], case["message"] = call(L, case, ledgers)
    close()
    applied = [case for case in cases if not case["status"] or ("refused" in case["message"] and "reason 9" not in case["message"])]
    assert part == "cpu" or not applied, applied    # every case of the gpu part ends in the host's checks
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(case, separators=(",", ":")) for case in cases) + "\n]\n")
    return cases


def load(part):
    with gzip.open(GOLDEN, "rt") as f:
        return [case for case in json.load(f) if case["part"] == part]


def join(paths):
    """the recorded parts as the golden file: one list, compressed without a time stamp"""
    cases = [case for path in paths for case in json.load(open(path))]
    with open(GOLDEN, "wb") as f, gzip.GzipFile(filename="", fileobj=f, mode="wb", mtime=0) as g:
        g.write(json.dumps(cases, separators=(",", ":")).encode())
    return cases


if __name__ == "__main__":
    got = join(sys.argv[2:]) if sys.argv[1] == "join" else record(sys.argv[1], sys.argv[2])
    print("%d cases, %d of them succeed, %d distinct messages" % (len(got), sum(not c["status"] for c in got), len({c["message"] for c in got})))
