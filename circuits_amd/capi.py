"""ctypes binding of include/hermez_witness.h (no torch types cross this boundary)."""
import ctypes
import os

R_MODULUS = 21888242871839275222246405745257275088548364400416034343698204186575808495617
_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    # HZ_WITNESS_LIB: alternative build of the same library (kernel tuning experiments)
    return os.environ.get("HZ_WITNESS_LIB") or os.path.join(_HERE, "libhermez_witness.so")


class HzError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("hz status %d: %s" % (status, msg))
        self.status = status


class ConstraintError(HzError):
    """A `===` of the circuit failed; message mirrors circom_runtime's text."""

    def __init__(self, instance, unit, cid, name, lhs, rhs):
        RuntimeError.__init__(self, "Constraint doesn't match %d != %d (%s, instance %d unit %d)" % (lhs, rhs, name, instance, unit))
        self.status = 3
        self.instance, self.unit, self.constraint_id, self.name, self.lhs, self.rhs = instance, unit, cid, name, lhs, rhs


def fr_to_bytes(vals):
    return b"".join(int(v % R_MODULUS).to_bytes(32, "little") for v in vals)


def fr_from_bytes(buf):
    buf = bytes(buf)
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


class hz_params(ctypes.Structure):
    _fields_ = [("template_id", ctypes.c_int32), ("nTx", ctypes.c_int32), ("nLevels", ctypes.c_int32),
                ("maxL1Tx", ctypes.c_int32), ("maxFeeTx", ctypes.c_int32), ("device", ctypes.c_int32),
                ("n_instances", ctypes.c_int32), ("flags", ctypes.c_int32)]


class hz_error(ctypes.Structure):
    _fields_ = [("instance", ctypes.c_int32), ("unit", ctypes.c_int32), ("constraint_id", ctypes.c_int32),
                ("lhs", ctypes.c_uint8 * 32), ("rhs", ctypes.c_uint8 * 32)]


class hz_symbol(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("index", ctypes.c_uint64)]


TEMPLATES = {"rollup-main": 0, "rollup-tx": 1, "decode-tx": 2, "fee-tx": 3, "hash-state": 4, "withdraw": 5, "hash-inputs": 6, "decode-float": 7, "compute-fee": 8, "fee-accumulator": 9, "balance-updater": 10,
             "rollup-tx-states": 11, "rq-tx-verifier": 12, "mux256": 13, "bits-compressed-2-ay-sign": 14, "ay-sign-2-ax": 15, "smt-processor": 16, "smt-verifier": 17}

# every symbol include/hermez_witness.h declares; tests check the .so exports all of them
EXPORTS = [
    "hz_version", "hz_last_error", "hz_device_count", "hz_ctx_create", "hz_ctx_destroy", "hz_witness_len", "hz_ctx_device_bytes", "hz_template_device_bytes",
    "hz_constraint_estimate", "hz_set_input", "hz_set_input_dev", "hz_copy_instance_inputs", "hz_inputs_packed_bytes", "hz_input_packed_width",
    "hz_input_packed_offset", "hz_host_alloc", "hz_host_free", "hz_inputs_upload", "hz_inputs_stage", "hz_inputs_stage_range", "hz_clear_inputs", "hz_input_count", "hz_input_name",
    "hz_witness_enqueue", "hz_witness_check", "hz_witness_run", "hz_witness_failures", "hz_witness_read", "hz_witness_dev_ptr",
    "hz_witness_total", "hz_witness_read_raw", "hz_ctx_set_profiling", "hz_profile_count", "hz_profile_get",
    "hz_ctx_set_shard", "hz_da_record_bytes", "hz_da_export", "hz_da_import", "hz_witness_enqueue_tail",
    "hz_witness_enqueue_tail_chain", "hz_sha_blocks", "hz_sha_state_bytes", "hz_sha_export", "hz_sha_expand",
    "hz_comm_create", "hz_comm_destroy", "hz_comm_rank", "hz_comm_world", "hz_shard_step", "hz_ctx_ntx",
    "hz_symmap_create", "hz_symmap_create_r1cs", "hz_symmap_solved", "hz_symmap_check_r1cs", "hz_symmap_save", "hz_symmap_load", "hz_symmap_destroy", "hz_symmap_nvars", "hz_symmap_unresolved", "hz_symmap_derived", "hz_witness_read_sym", "hz_witness_write_wtns_sym", "hz_witness_gather",
    "hz_symmap_from_index", "hz_component_major_index", "hz_symmap_upload", "hz_witness_export_dev", "hz_witness_export_range_dev", "hz_witness_export_host", "hz_symmap_dev_index", "hz_witness_derive_dev",
    "hz_symbol_count", "hz_symbol_get", "hz_symbol_lookup", "hz_constraint_name", "hz_poseidon_batch",
    "hz_poseidon_batch_dev", "hz_shard_range", "hz_set_inputs_json", "hz_witness_write_json", "hz_witness_write_wtns", "hz_symbols_write_sym", "hz_fr_ops", "hz_fr_raw_ops", "hz_poseidon_dag",
    "hz_state_create", "hz_state_destroy", "hz_state_load", "hz_state_root", "hz_state_apply", "hz_state_proofs", "hz_state_download", "hz_state_device_ms",
    "hz_smt_create", "hz_smt_destroy", "hz_smt_reset", "hz_smt_root", "hz_smt_size", "hz_smt_device_ms", "hz_smt_apply", "hz_smt_proofs", "hz_smt_plan",
    "hz_ledger_create", "hz_ledger_destroy", "hz_ledger_load", "hz_ledger_root", "hz_ledger_accounts", "hz_ledger_tree", "hz_ledger_apply_l2",
    "hz_ledger_outputs_dev", "hz_ledger_plan_l2", "hz_ledger_device_ms", "hz_ledger_semantic_ms",
    "hz_ledger_apply_l2_signed", "hz_ledger_verify_l2", "hz_ledger_sig_outputs_dev", "hz_ledger_sig_ms",
    "hz_ledger_apply_l2_addr", "hz_ledger_resolve_l2", "hz_ledger_aux_to_idx_dev", "hz_ledger_resolve_ms",
    "hz_ledger_apply_batch", "hz_ledger_plan_batch", "hz_ledger_l1_flags_dev", "hz_ledger_l1_ms",
    "hz_ledger_apply_batch_exits", "hz_ledger_exit_outputs_dev", "hz_ledger_exit_tree", "hz_ledger_exit_accounts", "hz_ledger_plan_exits", "hz_ledger_exit_ms",
    "hz_ledger_create_growing", "hz_ledger_load_accounts", "hz_ledger_size", "hz_ledger_last_idx", "hz_ledger_state_smt", "hz_ledger_apply_batch_creates",
    "hz_ledger_create_outputs_dev", "hz_ledger_create_ms", "hz_ledger_plan_creates",
    "hz_ledger_apply_batch_atomic", "hz_ledger_verify_l2_atomic", "hz_ledger_plan_atomic", "hz_ledger_rq_ms",
    "hz_ledger_select_batch", "hz_ledger_plan_select", "hz_ledger_select_ms",
    "hz_ledger_exit_keep", "hz_ledger_exit_forget", "hz_ledger_exit_kept", "hz_ledger_exit_archive_stats", "hz_ledger_exit_root_of", "hz_ledger_withdraw_rows",
    "hz_ledger_withdraw_rows_dev", "hz_ledger_withdraw_ms", "hz_ledger_exit_keep_ms",
    "hz_ledger_main_inputs", "hz_ledger_main_inputs_ms", "hz_ledger_plan_main_inputs",
    "hz_ledger_journal", "hz_ledger_applied", "hz_ledger_rollback", "hz_ledger_journal_stats", "hz_ledger_journal_ms", "hz_ledger_rollback_ms",
]


class hz_l2tx(ctypes.Structure):
    _fields_ = [("from_idx", ctypes.c_uint64), ("to_idx", ctypes.c_uint64), ("amount_f", ctypes.c_uint64), ("nonce", ctypes.c_uint64),
                ("token_id", ctypes.c_uint32), ("user_fee", ctypes.c_uint8)]


# hz_ledger_out's arrays in order: (name, rows per "tx" / "fee" / "one", columns "sib" / "fee" / None)
LEDGER_ARRAYS = (
    [(f + "1", "tx", None) for f in ("tokenID", "nonce", "sign", "balance", "ay", "ethAddr")] + [("siblings1", "tx", "sib")] +
    [(f + "2", "tx", None) for f in ("tokenID", "nonce", "sign", "balance", "ay", "ethAddr")] + [("siblings2", "tx", "sib")] +
    [("state_root_after", "tx", None), ("acc_fee_after", "tx", "fee")] +
    [(f + "3", "fee", None) for f in ("tokenID", "nonce", "sign", "balance", "ay", "ethAddr")] + [("siblings3", "fee", "sib")] +
    [("state_root_after_fee", "fee", None), ("final_acc_fee", "fee", None), ("old_root", "one", None), ("new_root", "one", None)])


class hz_l2sig(ctypes.Structure):
    _fields_ = [("s", ctypes.c_uint8 * 32), ("r8x", ctypes.c_uint8 * 32), ("r8y", ctypes.c_uint8 * 32), ("to_eth_addr", ctypes.c_uint8 * 32),
                ("to_bjj_ay", ctypes.c_uint8 * 32), ("max_num_batch", ctypes.c_uint32), ("to_bjj_sign", ctypes.c_uint8)]


# hz_ledger_sig_out's arrays in order, [m, 32] each
LEDGER_SIG_ARRAYS = ("tx_compressed_data", "tx_compressed_data_v2", "sig_l2_hash")
LEDGER_VERIFY_SIGS = 1   # hz_ledger_apply_l2_addr's flag


def l2sig_array(txs):
    """[{s, r8x, r8y, toEthAddr, toBjjAy, maxNumBatch, toBjjSign}] (builder's transaction dictionaries; missing keys are 0) -> hz_l2sig
    array. A value that does not fit its member is passed on truncated to 256 bits / as the library's argument error."""
    arr = (hz_l2sig * max(len(txs), 1))()
    for i, t in enumerate(txs):
        g = arr[i]
        for member, key in (("s", "s"), ("r8x", "r8x"), ("r8y", "r8y"), ("to_eth_addr", "toEthAddr"), ("to_bjj_ay", "toBjjAy")):
            getattr(g, member)[:] = list((int(t.get(key, 0)) % (1 << 256)).to_bytes(32, "little"))
        g.max_num_batch = t.get("maxNumBatch", 0)
        g.to_bjj_sign = min(int(t.get("toBjjSign", 0)), 255)
    return arr


class hz_l2rq(ctypes.Structure):
    _fields_ = [("rq_tx_compressed_data_v2", ctypes.c_uint8 * 32), ("rq_to_eth_addr", ctypes.c_uint8 * 32), ("rq_to_bjj_ay", ctypes.c_uint8 * 32),
                ("rq_offset", ctypes.c_uint8)]


LEDGER_RQ_REASON = 13   # the rq fields of a row are not its target's link fields
SELECT_MAX_POOL, SELECT_MAX_SLOTS = 4096, 4096   # HZ_SELECT_MAX_POOL, HZ_SELECT_MAX_SLOTS
SELECT_PARTNER, SELECT_FULL = 14, 15             # verdicts of hz_ledger_select_batch that are no refusal reasons
LEDGER_FEE_OVERFLOW = 16                         # HZ_LEDGER_FEE_OVERFLOW: the refusal reason of a fee of 2^128 or more


class hz_ledger_select_out(ctypes.Structure):
    _fields_ = [("verdict", ctypes.c_void_p), ("kept", ctypes.c_void_p), ("n_kept", ctypes.c_void_p), ("rq_offset", ctypes.c_void_p), ("aux_to_idx", ctypes.c_void_p),
                ("rounds", ctypes.c_void_p)]


def partner_array(txs):
    """the `partner` key of every transaction dictionary (a POOL index, missing or None: -1) as an int32 array, or None when no
    transaction has a partner"""
    import numpy as np
    vals = [t.get("partner") for t in txs]
    if all(v is None or v < 0 for v in vals):
        return None
    return np.array([-1 if v is None else v for v in vals], dtype=np.int32)


def select_compact(txs, result):
    """the kept transactions of a Ledger.select_batch result, in order, as copies that carry the rqOffset of the compacted batch"""
    return [dict(txs[i], rqOffset=result["rq_offset"][i]) for i in result["kept"]]


def l2rq_array(txs):
    """[{rqOffset, rqTxCompressedDataV2, rqToEthAddr, rqToBjjAy}] (builder's transaction dictionaries; missing keys are 0) -> hz_l2rq array,
    or None when no transaction holds any of them (the library then checks no link). The fields are passed on as given: explicit, never
    derived from a neighbour. A value that does not fit its member -- a field outside 0 .. 2^256 - 1, an offset outside 0 .. 255 -- raises
    ValueError: nothing is reduced or clamped on the way. What fits and is not valid (a field >= r, an offset above 7) is the library's
    to refuse."""
    keys = (("rq_tx_compressed_data_v2", "rqTxCompressedDataV2"), ("rq_to_eth_addr", "rqToEthAddr"), ("rq_to_bjj_ay", "rqToBjjAy"))
    if not any(t.get("rqOffset", 0) or any(t.get(key, 0) for _, key in keys) for t in txs):
        return None
    arr = (hz_l2rq * max(len(txs), 1))()
    for i, t in enumerate(txs):
        g = arr[i]
        for member, key in keys:
            v = int(t.get(key, 0))
            if not 0 <= v < 1 << 256:
                raise ValueError("tx %d: %s = %d does not fit 32 bytes" % (i, key, v))
            getattr(g, member)[:] = list(v.to_bytes(32, "little"))
        k = int(t.get("rqOffset", 0))
        if not 0 <= k <= 255:
            raise ValueError("tx %d: rqOffset = %d does not fit a byte" % (i, k))
        g.rq_offset = k
    return arr


class hz_l1tx(ctypes.Structure):
    _fields_ = [("from_idx", ctypes.c_uint64), ("to_idx", ctypes.c_uint64), ("amount_f", ctypes.c_uint64), ("load_amount_f", ctypes.c_uint64),
                ("token_id", ctypes.c_uint32), ("from_eth_addr", ctypes.c_uint8 * 32)]


LEDGER_MAX_L1 = 512   # HZ_LEDGER_MAX_L1
L1_NULLIFY_LOAD, L1_AMOUNT_NULLIFIED = 1, 2   # the bits of hz_ledger_apply_batch's flag bytes


# hz_ledger_exit_out's arrays in order: [rows, 32] each, the last [1, 32]
LEDGER_EXIT_ARRAYS = ("new_exit", "is_old0_2", "old_key2", "old_value2", "exit_root_after", "new_exit_root")


# hz_ledger_create_out's arrays in order: [rows, 32] each, the last [1, 32]
# hz_withdraw_rows_out's members in order: Withdraw's input signals, and the status bytes
WITHDRAW_ARRAYS = ("root_exit", "eth_addr", "token_id", "balance", "idx", "sign", "ay", "siblings_state", "status")
WITHDRAW_SIGNALS = {"root_exit": "rootExit", "eth_addr": "ethAddr", "token_id": "tokenID", "balance": "balance", "idx": "idx", "sign": "sign", "ay": "ay",
                    "siblings_state": "siblingsState"}
WITHDRAW_MAX_ROWS = 1 << 20
LEDGER_CREATE_ARRAYS = ("aux_from_idx", "is_old0_1", "old_key1", "old_value1", "out_idx_after", "new_last_idx")
# hz_ledger_plan_main_inputs: the kind flags of the call (HZ_MI_*), a descriptor's kinds (HZ_MI_KIND_*) and sources (HZ_MI_SRC_*)
MI_SIGS, MI_RQ, MI_EXITS, MI_CREATES, MI_AUX, MI_GROWING = 1, 2, 4, 8, 16, 32
MI_KINDS = ("zero", "copy", "broadcast", "txCompressedData", "txCompressedDataV2", "amountF", "fromIdx", "toIdx", "toBjjAy", "toEthAddr", "maxNumBatch", "onChain",
            "newAccount", "rqOffset", "rqTxCompressedDataV2", "rqToEthAddr", "rqToBjjAy", "s", "r8x", "r8y", "loadAmountF", "fromEthAddr", "fromBjjCompressed")
MI_SRC_NONE, MI_SRC_OUT, MI_SRC_EXIT, MI_SRC_CREATE, MI_SRC_AUX_TO_IDX, MI_SRC_GLOBALS, MI_SRC_FEE_IDXS, MI_SRC_FEE_PLAN_TOKENS, MI_SRC_ROWS, MI_SRC_KEYS = (
    0, 1, 32, 40, 48, 49, 50, 51, 52, 53)


def mi_source_name(src):
    """a descriptor's source as a word: an array of hz_ledger_out / _exit_out / _create_out by its name, or what of the request it reads"""
    if MI_SRC_OUT <= src < MI_SRC_OUT + len(LEDGER_ARRAYS):
        return LEDGER_ARRAYS[src - MI_SRC_OUT][0]
    if MI_SRC_EXIT <= src < MI_SRC_EXIT + len(LEDGER_EXIT_ARRAYS):
        return LEDGER_EXIT_ARRAYS[src - MI_SRC_EXIT]
    if MI_SRC_CREATE <= src < MI_SRC_CREATE + len(LEDGER_CREATE_ARRAYS):
        return LEDGER_CREATE_ARRAYS[src - MI_SRC_CREATE]
    return {MI_SRC_NONE: None, MI_SRC_AUX_TO_IDX: "auxToIdx", MI_SRC_GLOBALS: "globals", MI_SRC_FEE_IDXS: "fee_idxs", MI_SRC_FEE_PLAN_TOKENS: "fee_plan_tokens",
            MI_SRC_ROWS: "rows", MI_SRC_KEYS: "from_bjj"}[src]


def from_bjj_array(l1_txs):
    """fromBjjCompressed of every L1 transaction dictionary as [n_l1, 32] little-endian bytes (missing: 0), or None when no row creates an
    account (fromIdx == 0)"""
    import numpy as np
    if not any(not t.get("fromIdx", 0) for t in l1_txs):
        return None
    return np.frombuffer(b"".join((int(t.get("fromBjjCompressed", 0)) % (1 << 256)).to_bytes(32, "little") for t in l1_txs), dtype=np.uint8).reshape(-1, 32).copy()


def l1tx_array(txs):
    """[{fromIdx, toIdx, amountF, loadAmountF, tokenID, fromEthAddr}] (builder's L1 transaction dictionaries; missing keys are 0) -> hz_l1tx
    array. An address that does not fit 256 bits is passed on truncated; one above 160 bits is the library's argument error."""
    arr = (hz_l1tx * max(len(txs), 1))()
    for i, t in enumerate(txs):
        g = arr[i]
        g.from_idx, g.to_idx, g.amount_f, g.load_amount_f = t.get("fromIdx", 0), t.get("toIdx", 0), t.get("amountF", 0), t.get("loadAmountF", 0)
        g.token_id = t.get("tokenID", 0)
        g.from_eth_addr[:] = list((int(t.get("fromEthAddr", 0)) % (1 << 256)).to_bytes(32, "little"))
    return arr


def l2tx_array(txs):
    """[{fromIdx, toIdx, amountF, nonce, tokenID, userFee}] (builder's transaction dictionaries; missing keys are 0) -> hz_l2tx array"""
    arr = (hz_l2tx * max(len(txs), 1))()
    for i, t in enumerate(txs):
        arr[i] = hz_l2tx(t.get("fromIdx", 0), t.get("toIdx", 0), t.get("amountF", 0), t.get("nonce", 0), t.get("tokenID", 0), t.get("userFee", 0))
    return arr


# The arguments of the ledger's apply and verify calls, each with its ctype, and every call's list of them in the order of its prototype in
# include/hermez_witness.h. Lib takes the argtypes from here, Ledger._call the order in which it hands over what it has built.
LEDGER_ARG_TYPES = {"l": ctypes.c_void_p, "n_l1": ctypes.c_size_t, "l1": ctypes.c_void_p, "from_bjj": ctypes.c_void_p, "m": ctypes.c_size_t, "txs": ctypes.c_void_p,
                    "sigs": ctypes.c_void_p, "rq": ctypes.c_void_p, "flags": ctypes.c_uint32, "aux_to_idx": ctypes.c_void_p, "chain_id": ctypes.c_uint32,
                    "current_num_batch": ctypes.c_uint32, "F": ctypes.c_size_t, "fee_plan_tokens": ctypes.c_void_p, "fee_idxs": ctypes.c_void_p, "n_sib": ctypes.c_size_t,
                    "out": ctypes.c_void_p, "sig_out": ctypes.c_void_p, "aux_to_idx_out": ctypes.c_void_p, "l1_flags_out": ctypes.c_void_p, "exit_out": ctypes.c_void_p,
                    "create_out": ctypes.c_void_p, "verdict_out": ctypes.c_void_p}
_ADDR_TAIL = "flags aux_to_idx chain_id current_num_batch F fee_plan_tokens fee_idxs n_sib out sig_out aux_to_idx_out"   # hz_ledger_apply_l2_addr's, every later form's
LEDGER_CALLS = {fn: tuple(args.split()) for fn, args in {
    "hz_ledger_apply_l2": "l m txs F fee_plan_tokens fee_idxs n_sib out",
    "hz_ledger_apply_l2_signed": "l m txs sigs chain_id current_num_batch F fee_plan_tokens fee_idxs n_sib out sig_out",
    "hz_ledger_verify_l2": "l m txs sigs chain_id current_num_batch verdict_out sig_out",
    "hz_ledger_verify_l2_atomic": "l m txs sigs rq chain_id current_num_batch verdict_out sig_out",
    "hz_ledger_apply_l2_addr": "l m txs sigs " + _ADDR_TAIL,
    "hz_ledger_apply_batch": "l n_l1 l1 m txs sigs " + _ADDR_TAIL + " l1_flags_out",
    "hz_ledger_apply_batch_exits": "l n_l1 l1 m txs sigs " + _ADDR_TAIL + " l1_flags_out exit_out",
    "hz_ledger_apply_batch_creates": "l n_l1 l1 from_bjj m txs sigs " + _ADDR_TAIL + " l1_flags_out exit_out create_out",
    "hz_ledger_apply_batch_atomic": "l n_l1 l1 from_bjj m txs sigs rq " + _ADDR_TAIL + " l1_flags_out exit_out create_out"}.items()}


def _rows_and_fees(l1_txs, txs, fee_plan_tokens, fee_idxs):
    """the rows and the fee plan of a ledger call as C takes them: dictionaries become hz_l1tx / hz_l2tx arrays, prebuilt arrays pass as they
    are, the plan becomes uint32 [F] and uint64 [F] -> (l1 or None for l1_txs None, txs, fee_plan_tokens, fee_idxs)"""
    import numpy as np
    l1 = l1_txs if l1_txs is None or isinstance(l1_txs, ctypes.Array) else l1tx_array(l1_txs)
    arr = txs if isinstance(txs, ctypes.Array) else l2tx_array(txs)
    plan = np.ascontiguousarray(fee_plan_tokens, dtype=np.uint32)
    idxs = np.ascontiguousarray(fee_idxs, dtype=np.uint64)
    if idxs.size != plan.size:
        raise ValueError("fee_plan_tokens and fee_idxs differ in length")
    return l1, arr, plan, idxs


def _host_arrays(got, into, shapes, dtype, strict=False, only=None):
    """the host arrays a call writes into, for shapes [(name, shape)]: into[name] where `into` has it (strict: it must), a fresh zero array
    otherwise, each checked for its shape, dtype (a numpy.dtype) and contiguity and entered in `got` by its name -> their addresses in
    order; only: the names that are wanted at all, the others' addresses are None"""
    import numpy as np
    ptrs = []
    for name, shape in shapes:
        if only is not None and name not in only:
            ptrs.append(None)
            continue
        a = got[name] = into[name] if into is not None and (strict or name in into) else np.zeros(shape, dtype=dtype)
        assert a.shape == shape and a.dtype == dtype and a.flags.c_contiguous
        ptrs.append(a.ctypes.data)
    return ptrs


class Lib:
    """Loaded libhermez_witness.so. Raises if the HIP library has not been built."""

    def __init__(self, path=None):
        path = path or lib_path()
        if not os.path.exists(path):
            raise HzError(-1, "HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
        self.c = ctypes.CDLL(path)
        c = self.c
        c.hz_version.restype = ctypes.c_char_p
        c.hz_last_error.restype = ctypes.c_char_p
        c.hz_device_count.restype = ctypes.c_int32
        c.hz_poseidon_batch.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]
        c.hz_poseidon_batch_dev.argtypes = [ctypes.c_int32, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        c.hz_poseidon_dag.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        c.hz_fr_ops.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
        c.hz_fr_raw_ops.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
        c.hz_shard_range.argtypes = [ctypes.c_int32] * 3 + [ctypes.POINTER(ctypes.c_int32)] * 2
        c.hz_shard_range.restype = None
        vp, u64 = ctypes.c_void_p, ctypes.c_uint64
        c.hz_ctx_create.argtypes = [ctypes.POINTER(hz_params), ctypes.POINTER(vp)]
        c.hz_ctx_destroy.argtypes = [vp]
        c.hz_ctx_destroy.restype = None
        for f in ("hz_witness_len", "hz_ctx_device_bytes", "hz_template_device_bytes", "hz_constraint_estimate", "hz_witness_total", "hz_symbol_count"):
            getattr(c, f).argtypes = [vp]
            getattr(c, f).restype = u64
        c.hz_set_input.argtypes = [vp, ctypes.c_int32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        c.hz_set_input_dev.argtypes = [vp, ctypes.c_int32, ctypes.c_char_p, vp, ctypes.c_size_t, vp]
        c.hz_copy_instance_inputs.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp]
        c.hz_clear_inputs.argtypes = [vp]
        c.hz_clear_inputs.restype = None
        c.hz_inputs_packed_bytes.argtypes = [vp]
        c.hz_inputs_packed_bytes.restype = u64
        c.hz_input_packed_width.argtypes = [vp, ctypes.c_int32]
        c.hz_input_packed_offset.argtypes = [vp, ctypes.c_int32]
        c.hz_input_packed_offset.restype = u64
        c.hz_host_alloc.argtypes = [ctypes.c_size_t]
        c.hz_host_alloc.restype = vp
        c.hz_host_free.argtypes = [vp]
        c.hz_host_free.restype = None
        c.hz_inputs_upload.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_size_t, vp]
        c.hz_inputs_stage.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_size_t, vp]
        c.hz_inputs_stage_range.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp, ctypes.c_size_t, ctypes.c_size_t, vp]
        c.hz_input_count.argtypes = [vp]
        c.hz_input_name.argtypes = [vp, ctypes.c_int32, ctypes.POINTER(u64)]
        c.hz_input_name.restype = ctypes.c_char_p
        c.hz_witness_enqueue.argtypes = [vp, vp]
        c.hz_witness_check.argtypes = [vp, ctypes.POINTER(hz_error)]
        c.hz_witness_run.argtypes = [vp, ctypes.POINTER(hz_error)]
        c.hz_witness_failures.argtypes = [vp, ctypes.POINTER(hz_error), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        c.hz_witness_read.argtypes = [vp, ctypes.c_int32, u64, u64, vp]
        c.hz_witness_read_raw.argtypes = [vp, u64, u64, vp]
        c.hz_witness_dev_ptr.argtypes = [vp]
        c.hz_witness_dev_ptr.restype = vp
        c.hz_set_inputs_json.argtypes = [vp, ctypes.c_int32, ctypes.c_char_p, ctypes.c_size_t]
        c.hz_witness_write_json.argtypes = [vp, ctypes.c_int32, ctypes.c_char_p]
        c.hz_witness_write_wtns.argtypes = [vp, ctypes.c_int32, ctypes.c_char_p]
        c.hz_symbols_write_sym.argtypes = [vp, ctypes.c_char_p]
        c.hz_symbol_get.argtypes = [vp, u64, ctypes.POINTER(hz_symbol)]
        c.hz_symmap_create.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp)]
        c.hz_symmap_create_r1cs.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp)]
        c.hz_symmap_solved.argtypes = [vp]
        c.hz_symmap_solved.restype = u64
        c.hz_symmap_check_r1cs.argtypes = [vp, vp, ctypes.c_int32, ctypes.POINTER(u64), ctypes.POINTER(u64), u64]
        c.hz_symmap_save.argtypes = [vp, vp, ctypes.c_char_p]
        c.hz_symmap_load.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(vp)]
        c.hz_symmap_destroy.argtypes = [vp]
        c.hz_symmap_destroy.restype = None
        c.hz_symmap_nvars.argtypes = [vp]
        c.hz_symmap_nvars.restype = u64
        c.hz_symmap_unresolved.argtypes = [vp, u64, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_char_p)]
        c.hz_symmap_unresolved.restype = u64
        c.hz_witness_read_sym.argtypes = [vp, vp, ctypes.c_int32, u64, u64, vp]
        c.hz_witness_write_wtns_sym.argtypes = [vp, vp, ctypes.c_int32, ctypes.c_char_p]
        c.hz_witness_gather.argtypes = [vp, ctypes.c_int32, vp, u64, vp]
        c.hz_symmap_upload.argtypes = [vp, vp, ctypes.POINTER(u64)]
        c.hz_symmap_from_index.argtypes = [vp, vp, u64, ctypes.POINTER(vp)]
        c.hz_component_major_index.argtypes = [vp, vp, u64]
        c.hz_component_major_index.restype = u64
        c.hz_witness_export_dev.argtypes = [vp, vp, ctypes.c_int32, vp, vp]
        c.hz_witness_export_range_dev.argtypes = [vp, vp, ctypes.c_int32, ctypes.c_int32, vp, vp]
        c.hz_witness_export_host.argtypes = [vp, vp, ctypes.c_int32, u64, u64, vp]
        c.hz_symmap_dev_index.argtypes = [vp, vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(u64)]
        c.hz_witness_derive_dev.argtypes = [vp, vp, ctypes.c_int32, ctypes.POINTER(vp), vp]
        c.hz_symbol_lookup.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(u64)]
        c.hz_constraint_name.restype = ctypes.c_char_p
        c.hz_ctx_set_shard.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
        c.hz_da_record_bytes.argtypes = [vp]
        c.hz_da_record_bytes.restype = u64
        c.hz_da_export.argtypes = [vp, vp, vp]
        c.hz_da_import.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp, vp]
        c.hz_witness_enqueue_tail.argtypes = [vp, vp]
        c.hz_witness_enqueue_tail_chain.argtypes = [vp, vp]
        for f in ("hz_sha_blocks", "hz_sha_state_bytes"):
            getattr(c, f).argtypes = [vp]
            getattr(c, f).restype = u64
        c.hz_sha_export.argtypes = [vp, vp, vp]
        c.hz_sha_expand.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp, vp]
        c.hz_comm_create.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p, ctypes.POINTER(vp)]
        c.hz_comm_destroy.argtypes = [vp]
        c.hz_comm_destroy.restype = None
        c.hz_comm_rank.argtypes = [vp]
        c.hz_comm_world.argtypes = [vp]
        c.hz_shard_step.argtypes = [vp, vp, vp]
        c.hz_ctx_ntx.argtypes = [vp]
        c.hz_ctx_set_profiling.argtypes = [vp, ctypes.c_int32]
        c.hz_profile_count.argtypes = [vp]
        c.hz_profile_get.argtypes = [vp, ctypes.c_int32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(u64), ctypes.POINTER(u64)]
        sz = ctypes.c_size_t
        c.hz_state_create.argtypes = [ctypes.c_int32, ctypes.c_int32, u64, ctypes.POINTER(vp)]
        c.hz_state_destroy.argtypes = [vp]
        c.hz_state_destroy.restype = None
        c.hz_state_load.argtypes = [vp, vp, vp, vp, vp]
        c.hz_state_root.argtypes = [vp, vp]
        c.hz_state_apply.argtypes = [vp, sz, vp, vp, sz, vp, vp, vp, vp]
        c.hz_state_proofs.argtypes = [vp, sz, vp, sz, vp, vp]
        c.hz_state_download.argtypes = [vp, ctypes.POINTER(vp), vp]
        c.hz_state_device_ms.argtypes = [vp]
        c.hz_state_device_ms.restype = ctypes.c_double
        c.hz_smt_create.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(vp)]
        c.hz_smt_destroy.argtypes = [vp]
        c.hz_smt_destroy.restype = None
        c.hz_smt_reset.argtypes = [vp]
        c.hz_smt_root.argtypes = [vp, vp]
        c.hz_smt_size.argtypes = [vp]
        c.hz_smt_size.restype = u64
        c.hz_smt_device_ms.argtypes = [vp]
        c.hz_smt_device_ms.restype = ctypes.c_double
        c.hz_smt_apply.argtypes = [vp, sz, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]
        c.hz_smt_proofs.argtypes = [vp, sz, vp, sz, vp, vp, vp, vp, vp, vp]
        c.hz_smt_plan.argtypes = [sz, vp, sz, vp, vp, vp, vp]
        c.hz_ledger_create.argtypes = [ctypes.c_int32, ctypes.c_int32, u64, ctypes.POINTER(vp)]
        c.hz_ledger_destroy.argtypes = [vp]
        c.hz_ledger_destroy.restype = None
        c.hz_ledger_load.argtypes = [vp, vp, vp, vp, vp]
        c.hz_ledger_root.argtypes = [vp, vp]
        c.hz_ledger_accounts.argtypes = [vp, sz, vp, vp]
        c.hz_ledger_tree.argtypes = [vp]
        c.hz_ledger_tree.restype = vp
        for f, names in LEDGER_CALLS.items():
            getattr(c, f).argtypes = [LEDGER_ARG_TYPES[name] for name in names]
        c.hz_ledger_outputs_dev.argtypes = [vp, vp]
        c.hz_ledger_plan_l2.argtypes = [sz, vp, sz, vp, vp, ctypes.c_int32, u64, vp, vp, vp, vp, ctypes.POINTER(sz), vp, vp]
        u32 = ctypes.c_uint32
        c.hz_ledger_sig_outputs_dev.argtypes = [vp, vp]
        c.hz_ledger_resolve_l2.argtypes = [vp, sz, vp, vp, vp]
        c.hz_ledger_aux_to_idx_dev.argtypes = [vp, ctypes.POINTER(vp)]
        c.hz_ledger_plan_batch.argtypes = [sz, vp, sz, vp, sz, vp, vp, ctypes.c_int32, u64, vp, vp, vp, vp, ctypes.POINTER(sz), vp, vp, vp, vp, ctypes.POINTER(sz), vp]
        c.hz_ledger_l1_flags_dev.argtypes = [vp, ctypes.POINTER(vp)]
        c.hz_ledger_exit_outputs_dev.argtypes = [vp, vp]
        c.hz_ledger_exit_tree.argtypes = [vp]
        c.hz_ledger_exit_tree.restype = vp
        c.hz_ledger_exit_accounts.argtypes = [vp, sz, vp, vp]
        c.hz_ledger_plan_exits.argtypes = [sz, vp, sz, vp, sz, vp, vp, ctypes.c_int32, u64, sz, vp, vp, vp, ctypes.POINTER(sz), vp, vp, vp, ctypes.POINTER(sz), vp, vp,
                                           vp, vp, vp, vp, vp]
        c.hz_ledger_create_growing.argtypes = [ctypes.c_int32, u64, u64, ctypes.c_int32, ctypes.POINTER(vp)]
        c.hz_ledger_load_accounts.argtypes = [vp, u64, vp, vp, vp, vp]
        for f in ("hz_ledger_size", "hz_ledger_last_idx"):
            getattr(c, f).argtypes = [vp]
            getattr(c, f).restype = u64
        c.hz_ledger_state_smt.argtypes = [vp]
        c.hz_ledger_state_smt.restype = vp
        c.hz_ledger_create_outputs_dev.argtypes = [vp, vp]
        c.hz_ledger_plan_creates.argtypes = [sz, vp, vp, sz, vp, sz, vp, vp, ctypes.c_int32, u64, u64, u64, vp, vp, ctypes.POINTER(sz)]
        c.hz_ledger_plan_atomic.argtypes = [sz, sz, vp, vp, vp, vp, vp]
        c.hz_ledger_select_batch.argtypes = [vp, sz, vp, vp, sz, vp, vp, vp, vp, u32, u32, u32, sz, vp]
        c.hz_ledger_plan_select.argtypes = [sz, vp, sz, vp, vp, vp, vp, vp, vp, ctypes.POINTER(sz), vp, vp, vp]
        c.hz_ledger_exit_keep.argtypes = [vp, u32]
        c.hz_ledger_exit_forget.argtypes = [vp, u32]
        c.hz_ledger_exit_kept.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]
        c.hz_ledger_exit_archive_stats.argtypes = [vp] + [ctypes.POINTER(sz)] * 4
        c.hz_ledger_exit_root_of.argtypes = [vp, u32, vp]
        c.hz_ledger_withdraw_rows.argtypes = [vp, sz, vp, vp, ctypes.c_int32, vp]
        c.hz_ledger_withdraw_rows_dev.argtypes = [vp, vp]
        c.hz_ledger_main_inputs.argtypes = [vp, vp, u64, vp, sz]
        c.hz_ledger_plan_main_inputs.argtypes = [sz, vp, vp, vp, vp, u64, u32, u32, u32, u32, u32, vp, vp, vp, vp]
        c.hz_ledger_main_inputs_ms.argtypes = [vp]
        c.hz_ledger_main_inputs_ms.restype = ctypes.c_double
        c.hz_ledger_journal.argtypes = [vp, u32]
        c.hz_ledger_applied.argtypes = [vp, ctypes.POINTER(u64)]
        c.hz_ledger_rollback.argtypes = [vp, u64]
        c.hz_ledger_journal_stats.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(sz), ctypes.POINTER(u64), ctypes.POINTER(sz), ctypes.POINTER(sz)]
        for f in (c.hz_ledger_journal_ms, c.hz_ledger_rollback_ms):
            f.argtypes = [vp]
            f.restype = ctypes.c_double
        for f in ("hz_ledger_device_ms", "hz_ledger_semantic_ms", "hz_ledger_sig_ms", "hz_ledger_resolve_ms", "hz_ledger_l1_ms", "hz_ledger_exit_ms", "hz_ledger_create_ms",
                  "hz_ledger_rq_ms", "hz_ledger_select_ms", "hz_ledger_withdraw_ms", "hz_ledger_exit_keep_ms"):
            getattr(c, f).argtypes = [vp]
            getattr(c, f).restype = ctypes.c_double

    def _check(self, st):
        if st != 0:
            raise HzError(st, self.c.hz_last_error().decode())

    def version(self):
        return self.c.hz_version().decode()

    def device_count(self):
        return self.c.hz_device_count()

    def poseidon_batch(self, t, inputs, witness=False, device=0):
        """inputs: list of n lists of t-1 ints -> (digests, sbox_witness or None)."""
        n = len(inputs)
        flat = fr_to_bytes([x for row in inputs for x in row])
        out = ctypes.create_string_buffer(32 * max(n, 1))
        nsbox = 8 * t + [56, 57, 56, 60, 60, 63][t - 2]
        wit = ctypes.create_string_buffer(96 * nsbox * max(n, 1)) if witness else None
        self._check(self.c.hz_poseidon_batch(device, t, n, flat, out, wit))
        return fr_from_bytes(out.raw[:32 * n]), (wit.raw if witness else None)

    def poseidon_batch_bytes(self, t, n, in_bytes, device=0):
        """n permutations from a bytes-like of n * (t-1) canonical 32-byte elements -> bytes of n digests (no per-element Python)"""
        out = ctypes.create_string_buffer(32 * max(n, 1))
        buf = (ctypes.c_char * len(in_bytes)).from_buffer_copy(in_bytes) if not isinstance(in_bytes, bytes) else in_bytes
        self._check(self.c.hz_poseidon_batch(device, t, n, buf, out, None))
        return out.raw[:32 * n]

    def poseidon_batch_dev(self, t, n, d_in, d_out, d_wit=None, stream=None):
        self._check(self.c.hz_poseidon_batch_dev(t, n, d_in, d_out, d_wit, stream))

    def template_device_bytes(self, template, nTx=0, nLevels=0, maxL1Tx=0, maxFeeTx=0, n_instances=1):
        """device memory a context of this shape will hold (hz_template_device_bytes): no device needed"""
        p = hz_params(TEMPLATES[template], nTx, nLevels, maxL1Tx, maxFeeTx, 0, n_instances, 0)
        self.c.hz_template_device_bytes.restype = ctypes.c_uint64
        self.c.hz_template_device_bytes.argtypes = [ctypes.POINTER(hz_params)]
        return self.c.hz_template_device_bytes(ctypes.byref(p))

    def fr_ops(self, op, a, b=None, device=0):
        """out[i] = a[i] (op) b[i]; op: 0 add, 1 sub, 2 mul, 3 sqr, 4 inv, 5 a*b+a+b, 6 2a*(-b)."""
        n = len(a)
        out = ctypes.create_string_buffer(32 * max(n, 1))
        self._check(self.c.hz_fr_ops(device, op, n, fr_to_bytes(a), fr_to_bytes(b) if b is not None else None, out))
        return fr_from_bytes(out.raw[:32 * n])

    def fr_raw_ops(self, op, form, operands, device=0):
        """One fr.h routine on raw limbs (hz_fr_raw_ops, a self test): operands uint32[n_operands, n, 9] -> uint32[n, 9]. Element i runs
        on thread i of 256-thread workgroups (lane i % 64). form 0: the kernel built with HZ_FR_INLINE, 1: without it."""
        import numpy as np
        assert operands.dtype == np.uint32 and operands.ndim == 3 and operands.shape[2] == 9 and operands.flags.c_contiguous
        n = operands.shape[1]
        out = np.zeros((n, 9), dtype=np.uint32)
        self._check(self.c.hz_fr_raw_ops(device, op, form, n, operands.ctypes.data_as(ctypes.c_void_p), operands.shape[0], out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def poseidon_dag(self, vals, job_in, job_out, seg_t, seg_first, seg_count, device=0):
        """vals: bytearray of 32-byte elements (known values in, digests out); job_in uint32[n,6], job_out uint32[n];
        segments (seg_t uint32, seg_first / seg_count uint64) in execution order. Returns the device time in ms."""
        import numpy as np
        assert job_in.dtype == np.uint32 and job_out.dtype == np.uint32 and seg_t.dtype == np.uint32
        assert seg_first.dtype == np.uint64 and seg_count.dtype == np.uint64 and job_in.flags.c_contiguous
        buf = (ctypes.c_char * len(vals)).from_buffer(vals)
        ms = ctypes.c_double(0.0)
        self._check(self.c.hz_poseidon_dag(device, buf, len(vals) // 32, job_in.ctypes.data_as(ctypes.c_void_p), job_out.ctypes.data_as(ctypes.c_void_p),
                                           ctypes.c_uint64(len(job_out)), seg_t.ctypes.data_as(ctypes.c_void_p), seg_first.ctypes.data_as(ctypes.c_void_p),
                                           seg_count.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(len(seg_t)), ctypes.byref(ms)))
        return ms.value

    def ctx(self, template, **kw):
        return Ctx(self, template, **kw)

    def state(self, k, first_idx=256, device=0):
        return State(self, k, first_idx=first_idx, device=device)

    def smt(self, n_sib_max, device=0):
        return SparseTree(self, n_sib_max, device=device)

    def smt_plan(self, keys, n_sib):
        """hz_smt_plan, a diagnostic: the host planner alone on an empty tree (integers only, no device needed) -> dictionary of numpy
        arrays depth (of each op's leaf), fnc (1 insert, 0 update), old_key, is_old0"""
        import numpy as np
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        m = keys.size
        out = {"depth": np.zeros(m, dtype=np.uint32), "fnc": np.zeros(m, dtype=np.uint8), "old_key": np.zeros(m, dtype=np.uint64),
               "is_old0": np.zeros(m, dtype=np.uint8)}
        self._check(self.c.hz_smt_plan(m, keys.ctypes.data, n_sib, out["depth"].ctypes.data, out["fnc"].ctypes.data, out["old_key"].ctypes.data,
                                       out["is_old0"].ctypes.data))
        return out

    def ledger(self, k, first_idx=256, device=0):
        return Ledger(self, k, first_idx=first_idx, device=device)

    def ledger_growing(self, capacity, first_idx=256, n_sib_max=33, device=0):
        """a ledger that takes L1 rows which create accounts: room for `capacity` accounts, the state tree a sparse tree of n_sib_max"""
        return GrowingLedger(self, capacity, first_idx=first_idx, n_sib_max=n_sib_max, device=device)

    def ledger_plan_creates(self, l1_txs, txs, fee_plan_tokens, fee_idxs, capacity, size, first_idx=256, growing=True):
        """hz_ledger_plan_creates, a diagnostic: the running index of a batch whose L1 rows may create accounts (fromIdx == 0), and the
        argument errors of apply_batch_creates but the depth, for a ledger of `capacity` that holds `size` accounts; no device needed.
        -> {"aux_from_idx": [rows], "out_idx_after": [rows], "n_creates": int}"""
        import numpy as np
        l1, arr, plan, idxs = _rows_and_fees(l1_txs, txs, fee_plan_tokens, fee_idxs)
        bjj = from_bjj_array(l1_txs)
        n_l1, m = len(l1_txs), len(txs)
        aux, after = np.zeros(max(n_l1 + m, 1), dtype=np.uint64), np.zeros(max(n_l1 + m, 1), dtype=np.uint64)
        n = ctypes.c_size_t(0)
        self._check(self.c.hz_ledger_plan_creates(n_l1, ctypes.addressof(l1), bjj.ctypes.data if bjj is not None else None, m, ctypes.addressof(arr), plan.size,
                                                  plan.ctypes.data, idxs.ctypes.data, 1 if growing else 0, capacity, first_idx, size, aux.ctypes.data,
                                                  after.ctypes.data, ctypes.byref(n)))
        return {"aux_from_idx": aux[:n_l1 + m].tolist(), "out_idx_after": after[:n_l1 + m].tolist(), "n_creates": n.value}

    def ledger_plan_atomic(self, n_l1, txs, rq=None):
        """hz_ledger_plan_atomic, a diagnostic: where the atomic link of every L2 transaction points in a batch of n_l1 L1 rows and the
        transactions txs, and whether it holds; no device needed. txs: transaction dictionaries with the signed destination and rqOffset,
        rqTxCompressedDataV2, rqToEthAddr, rqToBjjAy; rq: a prebuilt hz_l2rq array instead. -> {"target_row": [m] (-1: the comparison is
        against zeros), "verdict": [m] (0 or 13)}"""
        import numpy as np
        arr, sigs = l2tx_array(txs), l2sig_array(txs)
        rq = l2rq_array(txs) if rq is None else rq
        m = len(txs)
        target, verdict = np.zeros(max(m, 1), dtype=np.int64), np.zeros(max(m, 1), dtype=np.uint8)
        self._check(self.c.hz_ledger_plan_atomic(n_l1, m, ctypes.addressof(arr), ctypes.addressof(sigs), ctypes.addressof(rq) if rq is not None else None,
                                                 target.ctypes.data, verdict.ctypes.data))
        return {"target_row": target[:m].tolist(), "verdict": verdict[:m].tolist()}

    def ledger_plan_select(self, l1_txs, txs, aux_to_idx=None, partner=None, kept=None):
        """hz_ledger_plan_select, a diagnostic: the local slots of a select_batch call -- the distinct accounts its L1 rows (a create row
        with its auxFromIdx as fromIdx) and its pool touch, by first appearance -- its argument errors, and, given kept (a flag per pool
        transaction), the closure step alone; no device needed. partner: [m] pool indices, default the dictionaries' `partner` keys.
        -> {"slot_sender", "slot_receiver": [n_l1 + m] (-1: none), "slot_account": [slots]} plus "forced", "rq_offset": [m] with kept"""
        import numpy as np
        l1, arr = l1tx_array(l1_txs), txs if isinstance(txs, ctypes.Array) else l2tx_array(txs)
        n_l1, m = len(l1_txs), len(txs)
        if partner is None and not isinstance(txs, ctypes.Array):
            partner = partner_array(txs)
        par = np.ascontiguousarray(partner, dtype=np.int32) if partner is not None else None
        aux = np.ascontiguousarray(aux_to_idx, dtype=np.uint64) if aux_to_idx is not None else None
        kin = np.ascontiguousarray(kept, dtype=np.uint8) if kept is not None else None
        for a in (par, aux, kin):
            if a is not None and a.size != m:
                raise ValueError("one entry per pool transaction")
        R = max(n_l1 + m, 1)
        ss, sr, acct = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32), np.zeros(2 * R, dtype=np.uint64)
        forced, off, n = np.zeros(max(m, 1), dtype=np.uint8), np.zeros(max(m, 1), dtype=np.uint8), ctypes.c_size_t(0)
        ptr = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
        self._check(self.c.hz_ledger_plan_select(n_l1, ctypes.addressof(l1), m, ctypes.addressof(arr), ptr(aux), ptr(par), ptr(kin), ss.ctypes.data, sr.ctypes.data,
                                                 ctypes.byref(n), acct.ctypes.data, forced.ctypes.data, off.ctypes.data))
        out = {"slot_sender": ss[:n_l1 + m].tolist(), "slot_receiver": sr[:n_l1 + m].tolist(), "slot_account": acct[:n.value].tolist()}
        if kin is not None:
            out.update(forced=forced[:m].tolist(), rq_offset=off[:m].tolist())
        return out

    def ledger_plan_l2(self, txs, fee_plan_tokens, fee_idxs, k, first_idx=256):
        """hz_ledger_plan_l2, a diagnostic: the host planner alone (integers only, no device needed). txs: transaction dictionaries or an
        hz_l2tx array. -> dictionary of numpy arrays: ev_sender / ev_receiver / fee_slot / last_event [m] (-1: none), account / prev_same
        [events]"""
        import numpy as np
        _, arr, plan, idxs = _rows_and_fees(None, txs, fee_plan_tokens, fee_idxs)
        m, F = len(txs), plan.size
        out = {n: np.zeros(m, dtype=np.int32) for n in ("ev_sender", "ev_receiver", "fee_slot", "last_event")}
        acct, prev, n_ev = np.zeros(2 * m + F, dtype=np.uint64), np.zeros(2 * m + F, dtype=np.int32), ctypes.c_size_t(0)
        self._check(self.c.hz_ledger_plan_l2(m, ctypes.addressof(arr), F, plan.ctypes.data, idxs.ctypes.data, k, first_idx, out["ev_sender"].ctypes.data,
                                             out["ev_receiver"].ctypes.data, out["fee_slot"].ctypes.data, out["last_event"].ctypes.data, ctypes.byref(n_ev),
                                             acct.ctypes.data, prev.ctypes.data))
        out["account"], out["prev_same"] = acct[:n_ev.value], prev[:n_ev.value]
        return out

    def ledger_plan_batch(self, l1_txs, txs, fee_plan_tokens, fee_idxs, k, first_idx=256):
        """hz_ledger_plan_batch, a diagnostic: ledger_plan_l2 over the n_l1 + m rows of a batch (L1 first), plus the local slots of the L1
        run: l1_slot_sender / l1_slot_receiver [n_l1] (-1: no receiver) and slot_account [slots]"""
        import numpy as np
        l1, arr, plan, idxs = _rows_and_fees(l1_txs, txs, fee_plan_tokens, fee_idxs)
        n_l1, m, F = len(l1_txs), len(txs), plan.size
        R = n_l1 + m
        out = {n: np.zeros(R, dtype=np.int32) for n in ("ev_sender", "ev_receiver", "fee_slot", "last_event")}
        out.update({n: np.zeros(n_l1, dtype=np.int32) for n in ("l1_slot_sender", "l1_slot_receiver")})
        acct, prev, n_ev = np.zeros(2 * R + F, dtype=np.uint64), np.zeros(2 * R + F, dtype=np.int32), ctypes.c_size_t(0)
        slot_acct, n_slots = np.zeros(max(2 * n_l1, 1), dtype=np.uint64), ctypes.c_size_t(0)
        self._check(self.c.hz_ledger_plan_batch(n_l1, ctypes.addressof(l1), m, ctypes.addressof(arr), F, plan.ctypes.data, idxs.ctypes.data, k, first_idx,
                                                out["ev_sender"].ctypes.data, out["ev_receiver"].ctypes.data, out["fee_slot"].ctypes.data,
                                                out["last_event"].ctypes.data, ctypes.byref(n_ev), acct.ctypes.data, prev.ctypes.data,
                                                out["l1_slot_sender"].ctypes.data, out["l1_slot_receiver"].ctypes.data, ctypes.byref(n_slots), slot_acct.ctypes.data))
        out["account"], out["prev_same"], out["slot_account"] = acct[:n_ev.value], prev[:n_ev.value], slot_acct[:n_slots.value]
        return out

    def ledger_plan_exits(self, l1_txs, txs, fee_plan_tokens, fee_idxs, k, n_sib=None, first_idx=256):
        """hz_ledger_plan_exits, a diagnostic: the plan of a batch whose rows may be exits (toIdx == 1), no device needed. An exit row makes
        its sender event and no receiver event; its operation on the exit tree is in a second ordered list. -> dictionary of numpy arrays:
        ev_sender / ev_receiver / last_event / ev_exit / last_exit [rows] (-1: none), account [events], and per exit operation exit_row,
        exit_key, exit_prev (-1: the operation is the insert), exit_perm (grouped by key), exit_insert, exit_is_old0, exit_old_key"""
        import numpy as np
        l1, arr, plan, idxs = _rows_and_fees(l1_txs, txs, fee_plan_tokens, fee_idxs)
        n_l1, m, F = len(l1_txs), len(txs), plan.size
        R = n_l1 + m
        out = {n: np.zeros(R, dtype=np.int32) for n in ("ev_sender", "ev_receiver", "last_event", "ev_exit", "last_exit")}
        acct, n_ev, n_x = np.zeros(2 * R + F, dtype=np.uint64), ctypes.c_size_t(0), ctypes.c_size_t(0)
        per_op = {"exit_row": np.uint32, "exit_key": np.uint64, "exit_prev": np.int32, "exit_perm": np.uint32, "exit_insert": np.uint8, "exit_is_old0": np.uint8,
                  "exit_old_key": np.uint64}
        ops = {n: np.zeros(max(R, 1), dtype=t) for n, t in per_op.items()}
        self._check(self.c.hz_ledger_plan_exits(n_l1, ctypes.addressof(l1), m, ctypes.addressof(arr), F, plan.ctypes.data, idxs.ctypes.data, k, first_idx,
                                                k + 1 if n_sib is None else n_sib, out["ev_sender"].ctypes.data, out["ev_receiver"].ctypes.data,
                                                out["last_event"].ctypes.data, ctypes.byref(n_ev), acct.ctypes.data, out["ev_exit"].ctypes.data,
                                                out["last_exit"].ctypes.data, ctypes.byref(n_x), *[ops[n].ctypes.data for n in per_op]))
        out["account"] = acct[:n_ev.value]
        out.update({n: a[:n_x.value] for n, a in ops.items()})
        return out

    def ledger_plan_main_inputs(self, layout, n_tx, n_levels, max_l1, max_fee, flags=0):
        """hz_ledger_plan_main_inputs: the descriptor table hz_ledger_main_inputs makes of a packed layout -- (total bytes, [(name, byte
        offset, element bytes, flat length)]) as Ctx.packed_layout gives it -- for RollupMain(n_tx, n_levels, max_l1, max_fee) and a call
        of the kind `flags` says (MI_SIGS | MI_RQ | MI_EXITS | MI_CREATES | MI_AUX | MI_GROWING)
        -> {signal: (kind word of MI_KINDS, source word of mi_source_name, first row, rows)}"""
        import numpy as np
        total, sigs = layout
        n = len(sigs)
        names = (ctypes.c_char_p * max(n, 1))(*[nm.encode() for nm, _, _, _ in sigs])
        offs = np.array([o for _, o, _, _ in sigs] or [0], dtype=np.uint64)
        widths = np.array([w for _, _, w, _ in sigs] or [0], dtype=np.uint32)
        lens = np.array([ln for _, _, _, ln in sigs] or [0], dtype=np.uint64)
        kind, src = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        r0, rows = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
        self._check(self.c.hz_ledger_plan_main_inputs(n, ctypes.addressof(names), offs.ctypes.data, widths.ctypes.data, lens.ctypes.data, total, n_tx, n_levels, max_l1,
                                                      max_fee, flags, kind.ctypes.data, src.ctypes.data, r0.ctypes.data, rows.ctypes.data))
        return {nm: (MI_KINDS[kind[i]], mi_source_name(int(src[i])), int(r0[i]), int(rows[i])) for i, (nm, _, _, _) in enumerate(sigs)}

    def host_alloc(self, nbytes):
        """pinned host memory for hz_inputs_upload (address as int); free with host_free"""
        p = self.c.hz_host_alloc(nbytes)
        if not p:
            raise HzError(2, self.c.hz_last_error().decode())
        return p

    def host_free(self, p):
        self.c.hz_host_free(p)

    def shard_range(self, n_tx, world, rank):
        f, c = ctypes.c_int32(), ctypes.c_int32()
        self.c.hz_shard_range(n_tx, world, rank, ctypes.byref(f), ctypes.byref(c))
        return f.value, c.value


class Comm:
    """hz_comm: one per rank. transport "rccl" (librccl.so loaded by the library with dlopen) or "socket" (host-staged over the rendezvous)"""

    def __init__(self, L, transport, rank, world, path=None, device=0):
        self.L = L
        self.h = ctypes.c_void_p()
        L._check(L.c.hz_comm_create({"rccl": 1, "socket": 2}[transport], device, rank, world, path.encode() if path else None, ctypes.byref(self.h)))

    def close(self):
        if self.h:
            self.L.c.hz_comm_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_inputs(layout, inputs):
    """The packed bulk-upload buffer (bytes) of one instance from an input object {signal: number | nested lists} and
    Ctx.packed_layout(). Pure Python: usable in worker processes that have no GPU."""
    total, sigs = layout
    out = bytearray(total)
    for name, off, width, flat_len in sigs:
        flat = _flatten(inputs[name])
        if len(flat) != flat_len:
            raise ValueError("input %s: expected %d values, got %d" % (name, flat_len, len(flat)))
        if width == 32:
            out[off:off + 32 * flat_len] = fr_to_bytes(flat)
        else:
            out[off:off + flat_len] = bytes(flat)
    return bytes(out)


def _flatten(v):
    if isinstance(v, (list, tuple)):
        out = []
        for x in v:
            out.extend(_flatten(x))
        return out
    return [int(v)]


class Ctx:
    """One circuit context (hz_ctx): the object the reference's `tester()` returns."""

    def __init__(self, L, template, nTx=0, nLevels=0, maxL1Tx=0, maxFeeTx=0, n_instances=1, device=0, flags=0):
        self.L = L
        self.h = ctypes.c_void_p()
        p = hz_params(TEMPLATES[template], nTx, nLevels, maxL1Tx, maxFeeTx, device, n_instances, flags)
        L._check(L.c.hz_ctx_create(ctypes.byref(p), ctypes.byref(self.h)))
        self.n_instances = n_instances

    def close(self):
        if self.h:
            self.L.c.hz_ctx_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def witness_len(self):
        return self.L.c.hz_witness_len(self.h)

    def total(self):
        return self.L.c.hz_witness_total(self.h)

    def device_bytes(self):
        """device memory of this context, buffers allocated on first use included (hz_ctx_device_bytes)"""
        return self.L.c.hz_ctx_device_bytes(self.h)

    def constraint_estimate(self):
        return self.L.c.hz_constraint_estimate(self.h)

    def input_names(self):
        n = self.L.c.hz_input_count(self.h)
        out = []
        for i in range(n):
            ln = ctypes.c_uint64()
            out.append((self.L.c.hz_input_name(self.h, i, ctypes.byref(ln)).decode(), ln.value))
        return out

    def set_input(self, name, value, instance=0):
        flat = _flatten(value)
        self.L._check(self.L.c.hz_set_input(self.h, instance, name.encode(), fr_to_bytes(flat), len(flat)))

    def set_inputs(self, d, instance=0):
        for k, v in d.items():
            self.set_input(k, v, instance)

    def set_input_dev(self, name, d_vals, count, instance=0, stream=None):
        """hz_set_input_dev: `count` canonical 32-byte elements that already lie in device memory (an address)"""
        self.L._check(self.L.c.hz_set_input_dev(self.h, instance, name.encode(), d_vals, count, stream))

    def packed_layout(self):
        """(total bytes, [(name, byte offset, element bytes, flat length)]) of the bulk-upload buffer of one instance"""
        total = self.L.c.hz_inputs_packed_bytes(self.h)
        if not total:
            raise HzError(2, self.L.c.hz_last_error().decode())
        return total, [(nm, self.L.c.hz_input_packed_offset(self.h, i), self.L.c.hz_input_packed_width(self.h, i), ln) for i, (nm, ln) in enumerate(self.input_names())]

    def upload(self, instance, packed, nbytes=None, stream=None):
        """hz_inputs_upload: `packed` is bytes / bytearray, or the address of a (pinned) host buffer of nbytes"""
        if isinstance(packed, (bytes, bytearray)):
            nbytes = len(packed)
            buf = (ctypes.c_char * nbytes).from_buffer_copy(packed)
            self.L._check(self.L.c.hz_inputs_upload(self.h, instance, ctypes.addressof(buf), nbytes, stream))
            self._keep = getattr(self, "_keep", [])[-63:] + [buf]   # pageable source: keep it alive until the copy has run
        else:
            self.L._check(self.L.c.hz_inputs_upload(self.h, instance, packed, nbytes, stream))

    def stage(self, instance, packed_addr, nbytes, stream=None):
        """hz_inputs_stage: the H2D copy alone (pinned source); the next enqueue scatters the staged instances"""
        self.L._check(self.L.c.hz_inputs_stage(self.h, instance, packed_addr, nbytes, stream))

    def stage_range(self, first, count, packed_addr, nbytes_each, stride=None, stream=None):
        """hz_inputs_stage_range: `count` consecutive instances, one copy when the host buffers are contiguous"""
        self.L._check(self.L.c.hz_inputs_stage_range(self.h, first, count, packed_addr, nbytes_each, nbytes_each if stride is None else stride, stream))

    def copy_instance_inputs(self, src, dst, stream=None):
        """Replicate the inputs of instance `src` onto instance `dst` on the device."""
        self.L._check(self.L.c.hz_copy_instance_inputs(self.h, src, dst, stream))

    def clear_inputs(self):
        self.L.c.hz_clear_inputs(self.h)

    def _raise(self, st, err):
        if st == 3:
            raise ConstraintError(err.instance, err.unit, err.constraint_id, self.L.c.hz_constraint_name(err.constraint_id).decode(),
                                  int.from_bytes(bytes(err.lhs), "little"), int.from_bytes(bytes(err.rhs), "little"))
        self.L._check(st)

    def run(self):
        err = hz_error()
        self._raise(self.L.c.hz_witness_run(self.h, ctypes.byref(err)), err)

    def enqueue(self, stream=None):
        self.L._check(self.L.c.hz_witness_enqueue(self.h, stream))

    def check(self):
        err = hz_error()
        self._raise(self.L.c.hz_witness_check(self.h, ctypes.byref(err)), err)

    def failures(self):
        """After run() / check(): the first violated constraint of every failing instance, ordered by instance, as
        (instance, unit, constraint_id, name, lhs, rhs) tuples (hz_witness_failures)."""
        n = ctypes.c_size_t(0)
        self.L._check(self.L.c.hz_witness_failures(self.h, None, 0, ctypes.byref(n)))
        if n.value == 0:
            return []
        arr = (hz_error * n.value)()
        self.L._check(self.L.c.hz_witness_failures(self.h, arr, n.value, ctypes.byref(n)))
        return [(e.instance, e.unit, e.constraint_id, self.L.c.hz_constraint_name(e.constraint_id).decode(),
                 int.from_bytes(bytes(e.lhs), "little"), int.from_bytes(bytes(e.rhs), "little")) for e in arr]

    def set_inputs_json(self, text, instance=0):
        b = text.encode() if isinstance(text, str) else text
        self.L._check(self.L.c.hz_set_inputs_json(self.h, instance, b, len(b)))

    def write_wtns(self, path, instance=0):
        self.L._check(self.L.c.hz_witness_write_wtns(self.h, instance, path.encode()))

    def write_json(self, path, instance=0):
        self.L._check(self.L.c.hz_witness_write_json(self.h, instance, path.encode()))

    def write_sym(self, path):
        self.L._check(self.L.c.hz_symbols_write_sym(self.h, path.encode()))

    def read(self, first, count, instance=0):
        buf = ctypes.create_string_buffer(32 * max(count, 1))
        self.L._check(self.L.c.hz_witness_read(self.h, instance, first, count, buf))
        return fr_from_bytes(buf.raw[:32 * count])

    def read_bytes(self, first, count, instance=0):
        """the same elements as read(), as 32-byte little-endian records (no Python integers: GB-sized compares)"""
        buf = ctypes.create_string_buffer(32 * max(count, 1))
        self.L._check(self.L.c.hz_witness_read(self.h, instance, first, count, buf))
        return buf.raw[:32 * count]

    def read_raw_bytes(self, first=0, count=None):
        count = self.total() - first if count is None else count
        buf = ctypes.create_string_buffer(32 * max(count, 1))
        self.L._check(self.L.c.hz_witness_read_raw(self.h, first, count, buf))
        return buf.raw[:32 * count]

    # -- multi-GPU intra-batch shard
    def set_shard(self, first, count, tail):
        self.L._check(self.L.c.hz_ctx_set_shard(self.h, first, count, 1 if tail else 0))

    def da_record_bytes(self):
        return self.L.c.hz_da_record_bytes(self.h)

    def da_export(self, d_buf, stream=None):
        self.L._check(self.L.c.hz_da_export(self.h, d_buf, stream))

    def da_import(self, first, count, d_buf, stream=None):
        self.L._check(self.L.c.hz_da_import(self.h, first, count, d_buf, stream))

    def enqueue_tail(self, stream=None):
        self.L._check(self.L.c.hz_witness_enqueue_tail(self.h, stream))

    def enqueue_tail_chain(self, stream=None):
        self.L._check(self.L.c.hz_witness_enqueue_tail_chain(self.h, stream))

    def sha_blocks(self):
        return self.L.c.hz_sha_blocks(self.h)

    def sha_state_bytes(self):
        return self.L.c.hz_sha_state_bytes(self.h)

    def sha_export(self, d_buf, stream=None):
        self.L._check(self.L.c.hz_sha_export(self.h, d_buf, stream))

    def sha_expand(self, first, count, d_buf=None, stream=None):
        self.L._check(self.L.c.hz_sha_expand(self.h, first, count, d_buf, stream))

    def shard_step(self, comm, stream):
        """hz_shard_step: one sharded pass on `stream` (a hipStream_t handle) through the communicator `comm` (Comm); then check()"""
        self.L._check(self.L.c.hz_shard_step(self.h, comm.h, stream))

    def set_profiling(self, on=True, exclusive=False):
        self.L._check(self.L.c.hz_ctx_set_profiling(self.h, (2 if exclusive else 1) if on else 0))

    def profile(self):
        """[(kernel, ms, algorithmic_bytes, units)] of the last enqueue (after check())."""
        out = []
        for i in range(self.L.c.hz_profile_count(self.h)):
            nm, ms, by, un = ctypes.c_char_p(), ctypes.c_float(), ctypes.c_uint64(), ctypes.c_uint64()
            self.L._check(self.L.c.hz_profile_get(self.h, i, ctypes.byref(nm), ctypes.byref(ms), ctypes.byref(by), ctypes.byref(un)))
            out.append((nm.value.decode(), ms.value, by.value, un.value))
        return out

    def dev_ptr(self):
        return self.L.c.hz_witness_dev_ptr(self.h)

    def lookup(self, name):
        idx = ctypes.c_uint64()
        if not self.L.c.hz_symbol_lookup(self.h, name.encode(), ctypes.byref(idx)):
            raise KeyError(name)
        return idx.value

    def get(self, name, instance=0):
        return self.read(self.lookup(name), 1, instance)[0]

    def import_sym(self, text, r1cs=None):
        """circom .sym text (and, optionally, the .r1cs bytes of the same compile: hz_symmap_create_r1cs) -> SymMap (the witness in the
        compiler's variable order)"""
        b = text.encode() if isinstance(text, str) else text
        h = ctypes.c_void_p()
        if r1cs is None:
            self.L._check(self.L.c.hz_symmap_create(self.h, b, len(b), ctypes.byref(h)))
        else:
            self.L._check(self.L.c.hz_symmap_create_r1cs(self.h, b, len(b), bytes(r1cs), len(r1cs), ctypes.byref(h)))
        return SymMap(self, h)

    def symmap_from_index(self, index):
        """hz_symmap_from_index: `index` a numpy uint64 array, variable v = stored signal index[v] (index[0] == 0)"""
        import numpy as np
        a = np.ascontiguousarray(index, dtype=np.uint64)
        h = ctypes.c_void_p()
        self.L._check(self.L.c.hz_symmap_from_index(self.h, a.ctypes.data, a.size, ctypes.byref(h)))
        return SymMap(self, h)

    def component_major_index(self):
        """hz_component_major_index -> numpy uint64 array"""
        import numpy as np
        n = self.L.c.hz_component_major_index(self.h, None, 0)
        a = np.empty(n, dtype=np.uint64)
        self.L.c.hz_component_major_index(self.h, a.ctypes.data, n)
        return a

    def load_symmap(self, path):
        """hz_symmap_load: a map written by SymMap.save for this template and shape"""
        h = ctypes.c_void_p()
        self.L._check(self.L.c.hz_symmap_load(self.h, path.encode(), ctypes.byref(h)))
        return SymMap(self, h)

    def symbol_count(self):
        return self.L.c.hz_symbol_count(self.h)

    def symbol(self, i):
        s = hz_symbol()
        self.L._check(self.L.c.hz_symbol_get(self.h, i, ctypes.byref(s)))
        return s.name.decode(), s.index


class _Resident:
    """a device-resident structure of the library behind its handle: created by `_create` (arguments, then the handle's address), destroyed
    by `_destroy`, its 32-byte root read by `_root` -- the names of three C functions"""
    _create = _destroy = _root = None

    def _open(self, L, *args):
        self.L = L
        self.h = ctypes.c_void_p()
        self.device = args[0] if args else 0   # every _create takes the device first
        L._check(getattr(L.c, self._create)(*args, ctypes.byref(self.h)))

    def close(self):
        if self.h:
            getattr(self.L.c, self._destroy)(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def root(self):
        out = (ctypes.c_uint8 * 32)()
        self.L._check(getattr(self.L.c, self._root)(self.h, out))
        return int.from_bytes(bytes(out), "little")


class State(_Resident):
    """hz_state: the account tree of N = 2^k consecutive accounts resident on the device (builder.DenseState's geometry). Field elements
    cross as numpy uint8 arrays of 32-byte little-endian canonical integers."""
    _create, _destroy, _root = "hz_state_create", "hz_state_destroy", "hz_state_root"

    def __init__(self, L, k, first_idx=256, device=0):
        self._open(L, device, k, first_idx)
        self.k, self.N, self.first_idx = k, 1 << k, first_idx

    @staticmethod
    def _fr(a, shape):
        import numpy as np
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.shape != shape:
            raise ValueError("expected an array of shape %s, got %s" % (shape, a.shape))
        return a

    def load(self, e0, balance, ay, eth_addr):
        """the four leaf fields as [N, 32] arrays indexed by account idx - first_idx; builds the whole tree on the device"""
        cols = [self._fr(a, (self.N, 32)) for a in (e0, balance, ay, eth_addr)]
        self.L._check(self.L.c.hz_state_load(self.h, *[a.ctypes.data for a in cols]))

    def apply(self, idx, fields, n_sib=None):
        """m ordered updates of existing accounts: idx [m] integers, fields [m, 4, 32] (e0, balance, ay, ethAddr). Returns a dictionary of
        numpy arrays: siblings [m, n_sib, 32] (root side first, zero beyond depth k), old_value / old_root / new_root [m, 32]."""
        import numpy as np
        n_sib = self.k if n_sib is None else n_sib
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        m = idx.size
        fields = self._fr(fields, (m, 4, 32))
        out = {"siblings": np.zeros((m, max(n_sib, 0), 32), dtype=np.uint8), "old_value": np.zeros((m, 32), dtype=np.uint8),
               "old_root": np.zeros((m, 32), dtype=np.uint8), "new_root": np.zeros((m, 32), dtype=np.uint8)}
        self.L._check(self.L.c.hz_state_apply(self.h, m, idx.ctypes.data, fields.ctypes.data, n_sib, out["siblings"].ctypes.data,
                                              out["old_value"].ctypes.data, out["old_root"].ctypes.data, out["new_root"].ctypes.data))
        return out

    def proofs(self, idx, n_sib=None):
        """membership proofs against the current root -> (siblings [n, n_sib, 32], state hashes [n, 32])"""
        import numpy as np
        n_sib = self.k if n_sib is None else n_sib
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        sib = np.zeros((idx.size, max(n_sib, 0), 32), dtype=np.uint8)
        val = np.zeros((idx.size, 32), dtype=np.uint8)
        self.L._check(self.L.c.hz_state_proofs(self.h, idx.size, idx.ctypes.data, n_sib, sib.ctypes.data, val.ctypes.data))
        return sib, val

    def download(self):
        """(levels, value) in DenseState's layout: levels[d] is [2^d, 32], value [N, 32]"""
        import numpy as np
        levels = [np.zeros((1 << d, 32), dtype=np.uint8) for d in range(self.k + 1)]
        value = np.zeros((self.N, 32), dtype=np.uint8)
        ptrs = (ctypes.c_void_p * (self.k + 1))(*[a.ctypes.data for a in levels])
        self.L._check(self.L.c.hz_state_download(self.h, ptrs, value.ctypes.data))
        return levels, value

    def device_ms(self):
        """device time of the last load / apply"""
        return self.L.c.hz_state_device_ms(self.h)


class _BorrowedState(State):
    """the hz_state inside a Ledger: proofs / download / root work on it; the ledger owns it"""

    def __init__(self, L, h, k, first_idx):
        self.L, self.h = L, ctypes.c_void_p(h)
        self.k, self.N, self.first_idx = k, 1 << k, first_idx

    def close(self):
        self.h = ctypes.c_void_p()


class Ledger(_Resident):
    """hz_ledger: an hz_state plus the resident leaf fields; L2 transfers and the batch's fee transactions computed and applied on the
    device. Field elements cross as numpy uint8 arrays of 32-byte little-endian canonical integers."""
    _create, _destroy, _root = "hz_ledger_create", "hz_ledger_destroy", "hz_ledger_root"

    def __init__(self, L, k, first_idx=256, device=0):
        self._open(L, device, k, first_idx)
        self.k, self.N, self.first_idx = k, 1 << k, first_idx

    def load(self, e0, balance, ay, eth_addr):
        cols = [State._fr(a, (self.N, 32)) for a in (e0, balance, ay, eth_addr)]
        self.L._check(self.L.c.hz_ledger_load(self.h, *[a.ctypes.data for a in cols]))

    def accounts(self, idx):
        """the resident leaf fields (e0, balance, ay, ethAddr) of the accounts idx -> [n, 4, 32]"""
        import numpy as np
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        out = np.zeros((idx.size, 4, 32), dtype=np.uint8)
        self.L._check(self.L.c.hz_ledger_accounts(self.h, idx.size, idx.ctypes.data, out.ctypes.data))
        return out

    def tree(self):
        """the tree as a capi.State, borrowed: proofs / download / root"""
        return _BorrowedState(self.L, self.L.c.hz_ledger_tree(self.h), self.k, self.first_idx)

    @staticmethod
    def shapes(m, F, n_sib):
        rows = {"tx": m, "fee": F, "one": 1}
        cols = {"sib": n_sib, "fee": F}
        return [(name, (rows[r], 32) if c is None else (rows[r], cols[c], 32)) for name, r, c in LEDGER_ARRAYS]

    def _call(self, fn, txs, fee_plan_tokens=(), fee_idxs=(), chain_id=0, current_num_batch=0, n_sib=None, verify=False, aux_to_idx=None, outputs=True, into=None,
              sigs=None, l1_txs=None, from_bjj=None, rq=None, verdict=None, only=None):
        """the one path of every apply and verify form to C: builds each argument LEDGER_CALLS[fn] names, once, and calls fn with them in
        its row's order. What a form's row does not name it does not get, so the public methods say which form they are and pass on what
        they were given. sigs None: built from the dictionaries, False: null. rq and from_bjj None: built from the dictionaries, null
        beside a prebuilt array of their rows; rq False: null. verdict: the verify forms' [max(m, 1)] bytes. only: the names wanted on
        the host (apply_resident) -- every other array's pointer stays null, and so does a group without a wanted one.
        -> the host arrays by name: hz_ledger_out's, the signature arrays (a form with a verify flag: when verified), auxToIdx, l1_flags,
        the exit arrays, the create arrays; `into` must hold the first two groups and may hold the rest."""
        import numpy as np
        row = LEDGER_CALLS[fn]
        named = frozenset(row)
        n_sib = self.k if n_sib is None else n_sib
        l1, arr, plan, idxs = _rows_and_fees(l1_txs, txs, fee_plan_tokens, fee_idxs)
        n_l1, m = 0 if l1_txs is None else len(l1_txs), len(txs)
        if "from_bjj" in named and from_bjj is None and not isinstance(l1_txs, ctypes.Array):
            from_bjj = from_bjj_array(l1_txs)
        if "sigs" in named and sigs is None:
            sigs = l2sig_array(txs)
        if "rq" in named and rq is None and not isinstance(txs, ctypes.Array):
            rq = l2rq_array(txs)
        aux = None
        if aux_to_idx is not None:
            aux = np.ascontiguousarray(aux_to_idx, dtype=np.uint64)
            if aux.size != m:
                raise ValueError("aux_to_idx: one entry per %stransaction" % ("L2 " if "l1" in named else ""))
        addr = lambda a: None if a is None or a is False else ctypes.addressof(a)   # noqa: E731
        data = lambda a: None if a is None else a.ctypes.data                        # noqa: E731
        args = {"l": self.h, "n_l1": n_l1, "l1": addr(l1), "from_bjj": data(from_bjj), "m": m, "txs": addr(arr), "sigs": addr(sigs), "rq": addr(rq),
                "flags": LEDGER_VERIFY_SIGS if verify else 0, "aux_to_idx": data(aux), "chain_id": chain_id, "current_num_batch": current_num_batch, "F": plan.size,
                "fee_plan_tokens": plan.ctypes.data, "fee_idxs": idxs.ctypes.data, "n_sib": n_sib, "verdict_out": data(verdict)}
        got, structs = {}, []   # structs: the structs of pointers, alive until C has returned like every local above
        if outputs:
            R, u8 = n_l1 + m, np.dtype(np.uint8)
            for arg in ("out", "sig_out", "aux_to_idx_out", "l1_flags_out", "exit_out", "create_out"):
                if arg not in named or (arg == "sig_out" and "flags" in named and not verify):   # C refuses sig_out without its verify flag
                    continue
                if arg == "out":
                    shapes = self.shapes(R, plan.size, min(max(n_sib, 0), 64))
                elif arg == "sig_out":
                    shapes = [(name, (m, 32)) for name in LEDGER_SIG_ARRAYS]
                elif arg == "aux_to_idx_out":
                    shapes = [("auxToIdx", (R, 32))]
                elif arg == "l1_flags_out":
                    shapes = [("l1_flags", (n_l1,))]
                else:   # [rows, 32] each, the last [1, 32]
                    names = LEDGER_EXIT_ARRAYS if arg == "exit_out" else LEDGER_CREATE_ARRAYS
                    shapes = [(name, (R, 32)) for name in names[:-1]] + [(names[-1], (1, 32))]
                ptrs = _host_arrays(got, into, shapes, u8, arg in ("out", "sig_out"), only)
                if arg in ("aux_to_idx_out", "l1_flags_out"):   # plain pointers, handed over only where there is a row to write
                    args[arg] = ptrs[0] if shapes[0][1][0] else None
                elif any(ptrs):
                    structs.append((ctypes.c_void_p * len(ptrs))(*ptrs))
                    args[arg] = ctypes.addressof(structs[-1])
        self.L._check(getattr(self.L.c, fn)(*[args.get(name) for name in row]))
        return got

    def _dev(self, fn, names):
        """{name: device pointer} of the struct of pointers the getter fn fills"""
        ptrs = (ctypes.c_void_p * len(names))()
        self.L._check(getattr(self.L.c, fn)(self.h, ctypes.addressof(ptrs)))
        return dict(zip(names, ptrs))

    def apply_l2(self, txs, fee_plan_tokens, fee_idxs, n_sib=None, outputs=True, into=None):
        """txs: transaction dictionaries (fromIdx, toIdx, amountF, nonce, tokenID, userFee) or an hz_l2tx array; fee_plan_tokens /
        fee_idxs: [F]. Returns a dictionary of numpy arrays named as hz_ledger_out's members (outputs=False: nothing is copied to the
        host, outputs_dev has them; into: a dictionary of arrays to fill instead of fresh ones)."""
        return self._call("hz_ledger_apply_l2", txs, fee_plan_tokens, fee_idxs, n_sib=n_sib, outputs=outputs, into=into)

    def outputs_dev(self):
        """device pointers of the last successful apply_l2's arrays, by name; valid until the ledger's next call"""
        return self._dev("hz_ledger_outputs_dev", [name for name, _, _ in LEDGER_ARRAYS])

    def apply_l2_signed(self, txs, fee_plan_tokens, fee_idxs, chain_id, current_num_batch, n_sib=None, outputs=True, into=None):
        """apply_l2 with every L2 signature verified on the device first, against the senders' resident keys. txs: transaction
        dictionaries that also hold s, r8x, r8y and optionally toEthAddr, toBjjAy, toBjjSign, maxNumBatch. Returns apply_l2's
        dictionary with tx_compressed_data, tx_compressed_data_v2 and sig_l2_hash ([m, 32]) added. A rejected signature refuses the
        batch with reason 7, an expired maxNumBatch with reason 8."""
        return self._call("hz_ledger_apply_l2_signed", txs, fee_plan_tokens, fee_idxs, chain_id, current_num_batch, n_sib, outputs=outputs, into=into)

    def verify_l2(self, txs, chain_id, current_num_batch, outputs=False):
        """the mempool filter: one verdict per transaction against the resident keys -- 0 accepted (or a NOP), 7 signature rejected, 8
        maxNumBatch expired -- as a uint8 array; nothing resident changes. outputs=True: (verdicts, the three signature arrays)"""
        return self._verify("hz_ledger_verify_l2", txs, chain_id, current_num_batch, outputs, False)

    def verify_l2_atomic(self, txs, chain_id, current_num_batch, outputs=False, rq=None):
        """verify_l2 over transactions that carry atomic links (rqOffset, rqTxCompressedDataV2, rqToEthAddr, rqToBjjAy): the list is a
        batch of its own, row i is transaction i, and 13 marks a transaction whose rq fields are not the link fields of the row its offset
        names; 7 and 8 come first where they hold. The message hashed is the one with the rq fields. rq: a prebuilt hz_l2rq array."""
        return self._verify("hz_ledger_verify_l2_atomic", txs, chain_id, current_num_batch, outputs, rq)

    def _verify(self, fn, txs, chain_id, current_num_batch, outputs, rq):
        import numpy as np
        verdict = np.zeros(max(len(txs), 1), dtype=np.uint8)
        sig_out = self._call(fn, txs, chain_id=chain_id, current_num_batch=current_num_batch, outputs=outputs, rq=rq, verdict=verdict)
        return (verdict[:len(txs)], sig_out) if outputs else verdict[:len(txs)]

    def sig_outputs_dev(self):
        """device pointers of the three signature arrays of the last successful apply_l2_signed / verify_l2, by name"""
        return self._dev("hz_ledger_sig_outputs_dev", LEDGER_SIG_ARRAYS)

    def apply_l2_addr(self, txs, fee_plan_tokens, fee_idxs, chain_id, current_num_batch, n_sib=None, verify=False, aux_to_idx=None, outputs=True, into=None, sigs=None):
        """apply_l2 over transactions whose toIdx may be 0: a receiver named by toEthAddr, or by the "any" address 2^160 - 1 plus toBjjAy /
        toBjjSign, is found on the device (the lowest index that holds it and the token) unless aux_to_idx ([m] indices) supplies it.
        verify=True: every signature is checked first as in apply_l2_signed, and its three arrays are returned as well. Returns
        apply_l2's dictionary plus auxToIdx ([m, 32]). Reasons 9 (no such account), 10 and 11 (a supplied receiver does not hold the
        signed address / key) refuse the batch. sigs: a prebuilt hz_l2sig array to go with a prebuilt hz_l2tx array."""
        return self._call("hz_ledger_apply_l2_addr", txs, fee_plan_tokens, fee_idxs, chain_id, current_num_batch, n_sib, verify, aux_to_idx, outputs, into, sigs)

    def apply_batch(self, l1_txs, txs, fee_plan_tokens, fee_idxs, chain_id, current_num_batch, n_sib=None, verify=False, aux_to_idx=None, outputs=True, into=None,
                    sigs=None):
        """a whole batch: the L1 transactions l1_txs (dictionaries with fromIdx, toIdx, amountF, loadAmountF, tokenID, fromEthAddr, or an
        hz_l1tx array: deposits, depositTransfers and forceTransfers on existing accounts, nullified as the circuit does), then the L2
        transactions txs exactly as apply_l2_addr takes them. Every per-transaction array has len(l1_txs) + len(txs) rows, L1 first.
        Returns apply_l2_addr's dictionary plus l1_flags (uint8 [n_l1]: bit 0 nullifyLoadAmount, bit 1 isAmountNullified). sigs=False: no
        hz_l2sig array is passed at all (allowed when nothing is verified and no L2 transaction names its receiver by address)."""
        return self._call("hz_ledger_apply_batch", txs, fee_plan_tokens, fee_idxs, chain_id, current_num_batch, n_sib, verify, aux_to_idx, outputs, into, sigs, l1_txs)

    def apply_batch_exits(self, l1_txs, txs, fee_plan_tokens, fee_idxs, chain_id, current_num_batch, n_sib=None, verify=False, aux_to_idx=None, outputs=True,
                          into=None, sigs=None):
        """apply_batch over rows that may be exits (toIdx == 1: an L2 exit, an L1 forceExit): the amount goes into the batch's exit tree at
        key fromIdx, an insert the first time and an update after. Returns apply_batch's dictionary plus new_exit, is_old0_2, old_key2,
        old_value2, exit_root_after ([rows, 32]) and new_exit_root ([1, 32]). exit_tree() and exit_accounts() read the tree and its leaves
        until the ledger's next batch."""
        return self._call("hz_ledger_apply_batch_exits", txs, fee_plan_tokens, fee_idxs, chain_id, current_num_batch, n_sib, verify, aux_to_idx, outputs, into, sigs,
                          l1_txs)

    def apply_batch_creates(self, l1_txs, txs, fee_plan_tokens, fee_idxs, chain_id, current_num_batch, n_sib=None, verify=False, aux_to_idx=None, outputs=True,
                            into=None, sigs=None, from_bjj=None):
        """apply_batch_exits over L1 rows that may create accounts (fromIdx == 0, the key in fromBjjCompressed): a growing ledger makes
        account last_idx + 1 for each, in row order, and every later row may name it. Returns apply_batch_exits' dictionary plus
        aux_from_idx, is_old0_1, old_key1, old_value1, out_idx_after ([rows, 32]) and new_last_idx ([1, 32]). from_bjj: the keys as a
        prebuilt [n_l1, 32] array (from_bjj_array) to go with a prebuilt hz_l1tx array."""
        return self._call("hz_ledger_apply_batch_creates", txs, fee_plan_tokens, fee_idxs, chain_id, current_num_batch, n_sib, verify, aux_to_idx, outputs, into, sigs,
                          l1_txs, from_bjj)

    def apply_batch_atomic(self, l1_txs, txs, fee_plan_tokens, fee_idxs, chain_id, current_num_batch, n_sib=None, verify=False, aux_to_idx=None, outputs=True,
                           into=None, sigs=None, from_bjj=None, rq=None):
        """apply_batch_creates over L2 transactions that may carry atomic links: rqOffset (0 .. 7) names a row of the batch, and
        rqTxCompressedDataV2, rqToEthAddr, rqToBjjAy -- explicit, what the signer committed to -- must equal that row's txCompressedDataV2
        and signed destination, or be zero where the offset is 0 or names an L1 row, a NOP or a place outside the batch. A mismatch refuses
        the batch with reason 13, verified or not; sig_l2_hash is the message with the rq fields. rq: a prebuilt hz_l2rq array
        (l2rq_array), False: none at all. Returns apply_batch_creates' dictionary."""
        return self._call("hz_ledger_apply_batch_atomic", txs, fee_plan_tokens, fee_idxs, chain_id, current_num_batch, n_sib, verify, aux_to_idx, outputs, into, sigs,
                          l1_txs, from_bjj, rq)

    def apply_resident(self, l1_txs, txs, fee_plan_tokens, fee_idxs, chain_id, current_num_batch, n_sib=None, verify=False, atomic=False, sigs=None, from_bjj=None,
                       rq=None):
        """apply_batch_atomic (atomic=True) or apply_batch_exits with every array left on the device -- what main_inputs packs -- but the
        few bytes the caller of a packed batch still needs on the host: -> {"l1_flags": uint8 [n_l1], "new_exit_root": [1, 32]}. Rows
        as dictionaries, or prebuilt: l1_txs an hz_l1tx array with from_bjj, txs an hz_l2tx array with sigs (False: none) and rq"""
        if sigs is None and isinstance(txs, ctypes.Array):   # prebuilt rows have no dictionaries to build signatures from
            sigs = False
        return self._call("hz_ledger_apply_batch_atomic" if atomic else "hz_ledger_apply_batch_exits", txs, fee_plan_tokens, fee_idxs, chain_id, current_num_batch,
                          n_sib, verify, sigs=sigs, l1_txs=l1_txs, from_bjj=from_bjj, rq=rq, only=("l1_flags", "new_exit_root"))

    def main_inputs(self, ctx, old_last_idx, d_packed=None):
        """hz_ledger_main_inputs: the packed input buffer of one instance of the RollupMain context `ctx` for the batch the last apply
        call (any but apply_l2) applied, written on the device. d_packed: the address of ctx.packed_layout()[0] bytes of device memory
        (a slot of a larger buffer, say), default a fresh torch.uint8 CUDA tensor. -> (address, bytes, the tensor or None): what
        Ctx.stage / stage_range / upload take"""
        nbytes = self.L.c.hz_inputs_packed_bytes(ctx.h)
        if not nbytes:
            raise HzError(2, self.L.c.hz_last_error().decode())
        buf = None
        if d_packed is None:
            import torch
            buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda:%d" % self.device)
            d_packed = buf.data_ptr()
        self.L._check(self.L.c.hz_ledger_main_inputs(self.h, ctx.h, old_last_idx, d_packed, nbytes))
        return d_packed, nbytes, buf

    def main_inputs_ms(self):
        """device time of k_ledger_main_inputs in the last main_inputs"""
        return self.L.c.hz_ledger_main_inputs_ms(self.h)

    def journal(self, depth):
        """hz_ledger_journal: keep an undo record of each of the last `depth` applies (0: off, the default); discards the records held"""
        self.L._check(self.L.c.hz_ledger_journal(self.h, depth))

    def applied(self):
        """hz_ledger_applied: the mark -- successful apply calls since the last load"""
        v = ctypes.c_uint64()
        self.L._check(self.L.c.hz_ledger_applied(self.h, ctypes.byref(v)))
        return v.value

    def rollback(self, mark):
        """hz_ledger_rollback: the ledger as it was when applied() gave `mark`"""
        self.L._check(self.L.c.hz_ledger_rollback(self.h, mark))

    def journal_stats(self):
        """hz_ledger_journal_stats -> {"depth", "records", "oldest_mark", "bytes_used", "bytes_reserved"}"""
        v = (ctypes.c_uint32(), ctypes.c_size_t(), ctypes.c_uint64(), ctypes.c_size_t(), ctypes.c_size_t())
        self.L._check(self.L.c.hz_ledger_journal_stats(self.h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("depth", "records", "oldest_mark", "bytes_used", "bytes_reserved"), (x.value for x in v)))

    def journal_ms(self):
        """device time of the journal's save kernels in the last apply (0.0 with the journal off)"""
        return self.L.c.hz_ledger_journal_ms(self.h)

    def rollback_ms(self):
        """device time of the last rollback"""
        return self.L.c.hz_ledger_rollback_ms(self.h)

    def rq_ms(self):
        """device time of the link kernel of the last apply_batch_atomic / verify_l2_atomic (0.0 when none ran)"""
        return self.L.c.hz_ledger_rq_ms(self.h)

    def select_batch(self, l1_txs, txs, chain_id, current_num_batch, max_keep=None, verify=False, partner=None, sigs=None, from_bjj=None, rq=None):
        """hz_ledger_select_batch: a batch chosen from the POOL txs, in order, behind the mandatory L1 rows (as apply_batch_atomic takes
        them): what is applicable after everything kept before it is kept, the rest dropped with a reason; nothing resident changes.
        partner: [m] pool indices (-1: none), default the dictionaries' `partner` keys; the rqOffset of a dictionary is not read, its rq
        fields are. max_keep: the room in the batch, default the pool's length. sigs: a prebuilt hz_l2sig array, False: none at all.
        -> {"verdict": [m] (0 kept or a NOP, a refusal reason, SELECT_PARTNER, SELECT_FULL), "kept": pool indices in order,
        "rq_offset": [m], "aux_to_idx": [m], "rounds": int}; select_compact(txs, result) are the rows to apply"""
        import numpy as np
        prebuilt = isinstance(l1_txs, ctypes.Array)
        l1 = l1_txs if prebuilt else l1tx_array(l1_txs)
        bjj = from_bjj if from_bjj is not None or prebuilt else from_bjj_array(l1_txs)
        arr = txs if isinstance(txs, ctypes.Array) else l2tx_array(txs)
        n_l1, m = len(l1_txs), len(txs)
        if not isinstance(txs, ctypes.Array):
            sigs = l2sig_array(txs) if sigs is None else sigs
            rq = l2rq_array(txs) if rq is None else rq
            partner = partner_array(txs) if partner is None else partner
        par = np.ascontiguousarray(partner, dtype=np.int32) if partner is not None else None
        if par is not None and par.size != m:
            raise ValueError("partner: one entry per pool transaction")
        n = max(m, 1)
        verdict, kept, off, aux = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint64)
        n_kept, rounds = ctypes.c_size_t(0), ctypes.c_uint32(0)
        out = hz_ledger_select_out(verdict.ctypes.data, kept.ctypes.data, ctypes.addressof(n_kept), off.ctypes.data, aux.ctypes.data, ctypes.addressof(rounds))
        self.L._check(self.L.c.hz_ledger_select_batch(self.h, n_l1, ctypes.addressof(l1), bjj.ctypes.data if bjj is not None else None, m, ctypes.addressof(arr),
                                                      ctypes.addressof(sigs) if sigs not in (None, False) else None,
                                                      ctypes.addressof(rq) if rq not in (None, False) else None, par.ctypes.data if par is not None else None,
                                                      LEDGER_VERIFY_SIGS if verify else 0, chain_id, current_num_batch, m if max_keep is None else max_keep,
                                                      ctypes.addressof(out)))
        return {"verdict": verdict[:m].tolist(), "kept": kept[:n_kept.value].tolist(), "rq_offset": off[:m].tolist(), "aux_to_idx": aux[:m].tolist(),
                "rounds": rounds.value}

    def select_ms(self):
        """device time of k_ledger_select in the last select_batch"""
        return self.L.c.hz_ledger_select_ms(self.h)

    def create_outputs_dev(self):
        """device pointers of the six create arrays of the last successful apply_batch_creates, by name; valid until the ledger's next call"""
        return self._dev("hz_ledger_create_outputs_dev", LEDGER_CREATE_ARRAYS)

    def create_ms(self):
        """device time of the two create kernels of the last apply_batch_creates"""
        return self.L.c.hz_ledger_create_ms(self.h)

    def size(self):
        """live accounts"""
        return self.L.c.hz_ledger_size(self.h)

    def last_idx(self):
        """first_idx + size - 1; first_idx - 1 when the ledger is empty"""
        return self.L.c.hz_ledger_last_idx(self.h)

    def exit_outputs_dev(self):
        """device pointers of the six exit arrays of the last successful apply_batch_exits, by name; valid until the ledger's next call"""
        return self._dev("hz_ledger_exit_outputs_dev", LEDGER_EXIT_ARRAYS)

    def exit_tree(self):
        """the exit tree of the last batch as a capi.SparseTree, borrowed: proofs / root / size"""
        return _BorrowedSparseTree(self.L, self.L.c.hz_ledger_exit_tree(self.h))

    def exit_accounts(self, keys):
        """the fields (e0, balance, ay, ethAddr) of the exit leaves at keys -> [n, 4, 32]; a key that is not in the exit tree raises"""
        import numpy as np
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros((keys.size, 4, 32), dtype=np.uint8)
        self.L._check(self.L.c.hz_ledger_exit_accounts(self.h, keys.size, keys.ctypes.data, out.ctypes.data))
        return out

    def exit_ms(self):
        """device time of the exit kernels plus the exit tree's update of the last apply_batch_exits (0.0 without an exit operation)"""
        return self.L.c.hz_ledger_exit_ms(self.h)

    def exit_keep(self, batch_num):
        """freezes the exit tree as it stands under batch_num (above every kept number); the live tree and the *_dev outputs stay"""
        self.L._check(self.L.c.hz_ledger_exit_keep(self.h, batch_num))

    def exit_forget(self, below_batch):
        """drops every kept batch with a number below below_batch"""
        self.L._check(self.L.c.hz_ledger_exit_forget(self.h, below_batch))

    def exit_kept(self):
        """the kept batch numbers, ascending"""
        import numpy as np
        n = ctypes.c_size_t()
        self.L._check(self.L.c.hz_ledger_exit_kept(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint32)
        self.L._check(self.L.c.hz_ledger_exit_kept(self.h, out.ctypes.data, n.value, ctypes.byref(n)))
        return out[:n.value].tolist()

    def exit_archive_stats(self):
        """{snapshots, slabs, bytes_used, bytes_reserved} of the archive of kept exit trees"""
        v = [ctypes.c_size_t() for _ in range(4)]
        self.L._check(self.L.c.hz_ledger_exit_archive_stats(self.h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("snapshots", "slabs", "bytes_used", "bytes_reserved"), (x.value for x in v)))

    def exit_root_of(self, batch_num):
        """the exit root of a kept batch as an int; a batch that is not kept raises"""
        out = (ctypes.c_uint8 * 32)()
        self.L._check(self.L.c.hz_ledger_exit_root_of(self.h, batch_num, ctypes.addressof(out)))
        return int.from_bytes(bytes(out), "little")

    def withdraw_rows(self, batch_nums, idxs, n_levels, outputs=True, into=None):
        """Withdraw(n_levels)'s inputs for the queries (batch_nums[i], idxs[i]) over the kept exit trees -> {name: array} by WITHDRAW_ARRAYS:
        seven [n, 32] arrays, siblings_state [n, n_levels + 1, 32] and status [n] (0 found, 1 batch not kept, 2 idx not in that tree, 3 the
        leaf needs n_levels + 1 or more siblings; the rows of such a query are zero). outputs=False: nothing is copied to the host
        (withdraw_rows_dev has the arrays); into: arrays to write into by name, the others are not copied"""
        import numpy as np
        b = np.ascontiguousarray(batch_nums, dtype=np.uint32)
        k = np.ascontiguousarray(idxs, dtype=np.uint64)
        if b.shape != k.shape or b.ndim != 1:
            raise ValueError("withdraw_rows: batch_nums and idxs are two lists of one length")
        n = b.size
        got = {}
        if into is not None:
            got = dict(into)
        elif outputs:
            got = {name: np.zeros((n, 32), dtype=np.uint8) for name in WITHDRAW_ARRAYS[:7]}
            got["siblings_state"] = np.zeros((n, max(n_levels + 1, 0), 32), dtype=np.uint8)
            got["status"] = np.zeros(n, dtype=np.uint8)
        ptrs = (ctypes.c_void_p * len(WITHDRAW_ARRAYS))(*[got[name].ctypes.data if name in got else None for name in WITHDRAW_ARRAYS])
        self.L._check(self.L.c.hz_ledger_withdraw_rows(self.h, n, b.ctypes.data, k.ctypes.data, n_levels, ctypes.addressof(ptrs) if got else None))
        return got

    def withdraw_rows_dev(self):
        """device pointers of the nine arrays of the last withdraw_rows, by name; valid until the ledger's next call"""
        return self._dev("hz_ledger_withdraw_rows_dev", WITHDRAW_ARRAYS)

    def withdraw_ms(self):
        """device time of the two kernels of the last withdraw_rows"""
        return self.L.c.hz_ledger_withdraw_ms(self.h)

    def exit_keep_ms(self):
        """device time of the copies of the last exit_keep"""
        return self.L.c.hz_ledger_exit_keep_ms(self.h)

    def l1_flags_dev(self):
        """device pointer of the [n_l1] flag bytes of the last successful apply_batch; valid until the ledger's next call"""
        p = ctypes.c_void_p()
        self.L._check(self.L.c.hz_ledger_l1_flags_dev(self.h, ctypes.byref(p)))
        return p.value

    def l1_ms(self):
        """device time of the L1 kernel of the last apply_batch (0.0 without an L1 run)"""
        return self.L.c.hz_ledger_l1_ms(self.h)

    def resolve_l2(self, txs):
        """the lookup alone: the index apply_l2_addr would find for every transaction as a uint64 array -- 0 for a NOP, for toIdx != 0 or
        when no account matches; nothing resident changes"""
        import numpy as np
        arr, sigs = l2tx_array(txs), l2sig_array(txs)
        m = len(txs)
        out = np.zeros(max(m, 1), dtype=np.uint64)
        self.L._check(self.L.c.hz_ledger_resolve_l2(self.h, m, ctypes.addressof(arr), ctypes.addressof(sigs), out.ctypes.data))
        return out[:m]

    def aux_to_idx_dev(self):
        """device pointer of the [m, 32] auxToIdx rows of the last successful apply_l2_addr; valid until the ledger's next call"""
        p = ctypes.c_void_p()
        self.L._check(self.L.c.hz_ledger_aux_to_idx_dev(self.h, ctypes.byref(p)))
        return p.value

    def resolve_ms(self):
        """device time of the two lookup kernels of the last apply_l2_addr / resolve_l2 (0.0 when none ran)"""
        return self.L.c.hz_ledger_resolve_ms(self.h)

    def sig_ms(self):
        """device time of the two signature kernels of the last apply_l2_signed / verify_l2"""
        return self.L.c.hz_ledger_sig_ms(self.h)

    def device_ms(self):
        """device time of the last apply_l2"""
        return self.L.c.hz_ledger_device_ms(self.h)

    def semantic_ms(self):
        """device time of the last apply_l2's semantic kernels alone (first kernel to the failure-word read)"""
        return self.L.c.hz_ledger_semantic_ms(self.h)


class GrowingLedger(Ledger):
    """hz_ledger_create_growing: a ledger whose state tree is a sparse tree and whose planes have room for `capacity` accounts, so that L1
    rows may create accounts (apply_batch_creates). Every call of Ledger works on it, over its live accounts; n_sib defaults to n_sib_max."""
    _create = "hz_ledger_create_growing"

    def __init__(self, L, capacity, first_idx=256, n_sib_max=33, device=0):
        self._open(L, device, capacity, first_idx, n_sib_max)
        self.capacity, self.first_idx, self.n_sib_max = capacity, first_idx, n_sib_max
        self.k = n_sib_max   # what the calls take as their default n_sib

    @property
    def N(self):
        return self.size()

    def load(self, *cols):
        raise TypeError("a growing ledger is loaded with load_accounts")

    def load_accounts(self, e0, balance, ay, eth_addr):
        """consecutive accounts from first_idx: four [n, 32] arrays, 0 <= n <= capacity (n == 0: the genesis state)"""
        import numpy as np
        cols = [np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 32) for a in (e0, balance, ay, eth_addr)]
        n = cols[0].shape[0]
        if any(c.shape != (n, 32) for c in cols):
            raise ValueError("load_accounts: four [n, 32] arrays")
        self.L._check(self.L.c.hz_ledger_load_accounts(self.h, n, *[c.ctypes.data for c in cols]))

    def tree(self):
        raise TypeError("a growing ledger has no dense tree: state_smt()")

    def state_smt(self):
        """the state tree as a capi.SparseTree, borrowed: proofs / root / size"""
        t = _BorrowedSparseTree(self.L, self.L.c.hz_ledger_state_smt(self.h))
        t.n_sib_max = self.n_sib_max
        return t


class SparseTree(_Resident):
    """hz_smt: a circomlib sparse Merkle tree resident on the device that accepts inserts and updates (the exit tree; the state tree under
    create-account deposits). Field elements cross as numpy uint8 arrays of 32-byte little-endian canonical integers."""
    _create, _destroy, _root = "hz_smt_create", "hz_smt_destroy", "hz_smt_root"

    def __init__(self, L, n_sib_max, device=0):
        self._open(L, device, n_sib_max)
        self.n_sib_max = n_sib_max

    def reset(self):
        """the empty tree again; the device pools are kept"""
        self.L._check(self.L.c.hz_smt_reset(self.h))

    def size(self):
        """keys held"""
        return self.L.c.hz_smt_size(self.h)

    def apply(self, keys, fields, n_sib=None):
        """m ordered ops, each an insert (key absent) or an update (key present): keys [m] integers, fields [m, 4, 32] (e0, balance, ay,
        ethAddr). Returns a dictionary of numpy arrays, the inputs of SMTProcessor(n_sib) per op: siblings [m, n_sib, 32] (zero-padded),
        old_key [m], old_value [m, 32], is_old0 [m], fnc [m] (1 insert: fnc = [1, 0]; 0 update: fnc = [0, 1]), old_root / new_root [m, 32]."""
        import numpy as np
        n_sib = self.n_sib_max if n_sib is None else n_sib
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        m = keys.size
        fields = State._fr(fields, (m, 4, 32))
        out = {"siblings": np.zeros((m, min(max(n_sib, 0), 64), 32), dtype=np.uint8), "old_key": np.zeros(m, dtype=np.uint64),
               "old_value": np.zeros((m, 32), dtype=np.uint8), "is_old0": np.zeros(m, dtype=np.uint8), "fnc": np.zeros(m, dtype=np.uint8),
               "old_root": np.zeros((m, 32), dtype=np.uint8), "new_root": np.zeros((m, 32), dtype=np.uint8)}
        self.L._check(self.L.c.hz_smt_apply(self.h, m, keys.ctypes.data, fields.ctypes.data, n_sib, out["siblings"].ctypes.data, out["old_key"].ctypes.data,
                                            out["old_value"].ctypes.data, out["is_old0"].ctypes.data, out["fnc"].ctypes.data,
                                            out["old_root"].ctypes.data, out["new_root"].ctypes.data))
        return out

    def proofs(self, keys, n_sib=None):
        """membership / non-membership proofs against the current root (SMTVerifier's inputs) -> dictionary of numpy arrays: siblings
        [n, n_sib, 32], found [n], value [n, 32] (found keys), not_found_key [n], not_found_value [n, 32], is_old0 [n] (absent keys)"""
        import numpy as np
        n_sib = self.n_sib_max if n_sib is None else n_sib
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n = keys.size
        out = {"siblings": np.zeros((n, min(max(n_sib, 0), 64), 32), dtype=np.uint8), "found": np.zeros(n, dtype=np.uint8),
               "value": np.zeros((n, 32), dtype=np.uint8), "not_found_key": np.zeros(n, dtype=np.uint64),
               "not_found_value": np.zeros((n, 32), dtype=np.uint8), "is_old0": np.zeros(n, dtype=np.uint8)}
        self.L._check(self.L.c.hz_smt_proofs(self.h, n, keys.ctypes.data, n_sib, out["siblings"].ctypes.data, out["found"].ctypes.data, out["value"].ctypes.data,
                                             out["not_found_key"].ctypes.data, out["not_found_value"].ctypes.data, out["is_old0"].ctypes.data))
        return out

    def device_ms(self):
        """device time of the last apply"""
        return self.L.c.hz_smt_device_ms(self.h)


class _BorrowedSparseTree(SparseTree):
    """the hz_smt inside a Ledger, its exit tree: proofs / root / size work on it; the ledger owns it"""

    def __init__(self, L, h):
        self.L, self.h = L, ctypes.c_void_p(h)
        self.n_sib_max = 64

    def close(self):
        self.h = ctypes.c_void_p()


class SymMap:
    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def __del__(self):
        try:
            self.ctx.L.c.hz_symmap_destroy(self.h)
        except Exception:
            pass

    def nvars(self):
        return self.ctx.L.c.hz_symmap_nvars(self.h)

    def unresolved(self):
        """[(variable, a label)] of the variables none of whose labels the layout stores"""
        out = []
        n = self.ctx.L.c.hz_symmap_unresolved(self.h, 0, None, None)
        for i in range(n):
            v, nm = ctypes.c_uint64(), ctypes.c_char_p()
            self.ctx.L.c.hz_symmap_unresolved(self.h, i, ctypes.byref(v), ctypes.byref(nm))
            out.append((v.value, nm.value.decode()))
        return out

    def save(self, path):
        self.ctx.L._check(self.ctx.L.c.hz_symmap_save(self.ctx.h, self.h, path.encode()))

    def solved(self):
        """variables defined by the linear constraints of the .r1cs (hz_symmap_create_r1cs)"""
        return self.ctx.L.c.hz_symmap_solved(self.h)

    def check_r1cs(self, instance=0, cap=16):
        """(number of violated constraints, indices of the first `cap`) of the map's .r1cs on the witness it serves"""
        n, first = ctypes.c_uint64(), (ctypes.c_uint64 * cap)()
        self.ctx.L._check(self.ctx.L.c.hz_symmap_check_r1cs(self.ctx.h, self.h, instance, ctypes.byref(n), first, cap))
        return n.value, list(first[:min(cap, n.value)])

    def derived(self):
        """variables evaluated from stored signals by a rule (linear signals an unreduced compile keeps)"""
        f = self.ctx.L.c.hz_symmap_derived
        f.restype, f.argtypes = ctypes.c_uint64, [ctypes.c_void_p]
        return f(self.h)

    def read(self, first=0, count=None, instance=0):
        count = self.nvars() - first if count is None else count
        buf = ctypes.create_string_buffer(32 * max(count, 1))
        self.ctx.L._check(self.ctx.L.c.hz_witness_read_sym(self.ctx.h, self.h, instance, first, count, buf))
        return fr_from_bytes(buf.raw[:32 * count])

    def write_wtns(self, path, instance=0):
        self.ctx.L._check(self.ctx.L.c.hz_witness_write_wtns_sym(self.ctx.h, self.h, instance, path.encode()))

    def read_small(self, first, count, instance=0):
        """hz_witness_read_sym in pieces small enough to stay on its host evaluator (the independent route the device export is
        compared with in tests)"""
        out = []
        for f in range(first, first + count, 4096):
            out += self.read(f, min(4096, first + count - f), instance)
        return out

    def upload(self):
        """hz_symmap_upload: the map's device tables for this context; returns their size in bytes"""
        n = ctypes.c_uint64()
        self.ctx.L._check(self.ctx.L.c.hz_symmap_upload(self.ctx.h, self.h, ctypes.byref(n)))
        return n.value

    def export_dev(self, d_out, instance=0, stream=None):
        """hz_witness_export_dev: the witness of `instance` (-1: every instance) in this map's variable order into device memory"""
        self.ctx.L._check(self.ctx.L.c.hz_witness_export_dev(self.ctx.h, self.h, instance, d_out, stream))

    def export_host(self, instance=0, first=0, count=None, out=None):
        """hz_witness_export_host -> bytes (or into the caller's buffer address `out`)"""
        count = self.nvars() - first if count is None else count
        if out is not None:
            self.ctx.L._check(self.ctx.L.c.hz_witness_export_host(self.ctx.h, self.h, instance, first, count, out))
            return None
        buf = ctypes.create_string_buffer(32 * max(count, 1))
        self.ctx.L._check(self.ctx.L.c.hz_witness_export_host(self.ctx.h, self.h, instance, first, count, buf))
        return buf.raw[:32 * count]

    def dev_index(self):
        """hz_symmap_dev_index -> (device pointer to u64 phys0[nvars], device pointer to u32 inst_stride[nvars], derived slots)"""
        a, b, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()
        self.ctx.L._check(self.ctx.L.c.hz_symmap_dev_index(self.ctx.h, self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)))
        return a.value, b.value, n.value

    def derive_dev(self, instance=0, stream=None):
        p = ctypes.c_void_p()
        self.ctx.L._check(self.ctx.L.c.hz_witness_derive_dev(self.ctx.h, self.h, instance, ctypes.byref(p), stream))
        return p.value


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = Lib()
    return _lib
