/* hermez_witness.h -- C ABI of the MI355X-native witness generator for the Hermez rollup circuits.
 *
 * This is the drop-in boundary for the one hot path this repository accelerates: witness
 * calculation for the circuits of hermeznetwork/circuits. What each entry point replaces:
 *
 *   reference call site                                         replaced by
 *   ----------------------------------------------------------  --------------------------------
 *   circuit = await tester(path)          test/rollup-main.test.js:52,  test/rollup-tx.test.js:43
 *        (circom compile + WitnessCalculator instantiate)       hz_ctx_create / hz_ctx_destroy
 *   WitnessCalculator setSignal(name, idx, value) loop inside
 *        circuit.calculateWitness(input)  test/helpers/helpers.js:142,149    hz_set_input
 *   calculateWitness body (component code of DecodeTx/RollupTx/FeeTx/HashInputs,
 *        src/rollup-main.circom:201-475)                        hz_witness_run
 *   returned witness array w[]            test/helpers/helpers.js:149        hz_witness_read
 *   circuit.assertOut / getSignal via .sym                      hz_symbol_count / hz_symbol_get /
 *                                         test/helpers/helpers.js:143,154,170    hz_symbol_lookup
 *   native witness binary `./circuit input.json witness.json`   the same five calls
 *                                         tools/helpers/actions.js:132-146
 *   Poseidon(n) gadget (circomlib 0.5.2 poseidon.circom; call sites src/lib/hash-state.circom:32,
 *        src/decode-tx.circom:275)                              hz_poseidon_batch(_dev)
 *
 * All field elements cross this boundary as 32-byte little-endian canonical integers (< r), the
 * element format of snarkjs .wtns files. Plain C types only; caller-allocated buffers; no
 * exceptions cross the ABI. A context is used by one thread at a time.
 * There is NO CPU fallback: every entry point that computes returns HZ_ERR_NODEVICE when no
 * gfx950 device is usable.
 *
 * Streams. Every `void* stream` argument is a hipStream_t. NULL never means HIP's legacy default stream: it means the
 * context's own non-blocking stream, in every entry point alike. Asynchronous input writes (hz_set_input_dev,
 * hz_copy_instance_inputs, hz_inputs_upload) are ordered before the next hz_witness_enqueue / hz_witness_run of the same
 * context on whatever stream that call uses (an event, no host synchronisation). Everything else follows stream order:
 * hz_da_export / hz_da_import / hz_witness_enqueue_tail must be given the stream of the hz_witness_enqueue they follow, and a
 * collective between them must be ordered on that stream by the caller.
 */
#ifndef HERMEZ_WITNESS_H
#define HERMEZ_WITNESS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HZ_FR_BYTES 32

typedef enum {
    HZ_OK = 0,
    HZ_ERR_ARG = 1,        /* bad parameter */
    HZ_ERR_HIP = 2,        /* HIP runtime failure, see hz_last_error() */
    HZ_ERR_CONSTRAINT = 3, /* a `===` of the circuit does not hold; details in hz_error */
    HZ_ERR_INPUT = 4,      /* unknown / mis-shaped / missing input signal */
    HZ_ERR_NODEVICE = 5    /* no usable gfx950 device */
} hz_status;

/* main component selector: the templates the reference's suites instantiate as `component main` */
typedef enum {
    HZ_T_ROLLUP_MAIN = 0, /* RollupMain(nTx,nLevels,maxL1Tx,maxFeeTx)  src/rollup-main.circom:82   */
    HZ_T_ROLLUP_TX = 1,   /* RollupTx(nLevels,maxFeeTx)                src/rollup-tx.circom:78     */
    HZ_T_DECODE_TX = 2,   /* DecodeTx(nLevels)                         src/decode-tx.circom:44     */
    HZ_T_FEE_TX = 3,      /* FeeTx(nLevels)                            src/fee-tx.circom:26        */
    HZ_T_HASH_STATE = 4,  /* HashState()                               src/lib/hash-state.circom:18*/
    HZ_T_WITHDRAW = 5,    /* Withdraw(nLevels)                         src/withdraw.circom:21      */
    HZ_T_HASH_INPUTS = 6, /* HashInputs(nLevels,nTx,maxL1Tx,maxFeeTx)  src/hash-inputs.circom:23   */
    /* gadget mains of the reference's unit suites (one witness per instance, a single small kernel) */
    HZ_T_DECODE_FLOAT = 7,     /* DecodeFloat()                        src/lib/decode-float.circom:51   */
    HZ_T_COMPUTE_FEE = 8,      /* ComputeFee()                         src/compute-fee.circom:12        */
    HZ_T_FEE_ACCUMULATOR = 9,  /* FeeAccumulator(maxFeeTx)             src/fee-accumulator.circom:56    */
    HZ_T_BALANCE_UPDATER = 10, /* BalanceUpdater()                     src/balance-updater.circom:24    */
    HZ_T_ROLLUP_TX_STATES = 11,/* RollupTxStates()                     src/rollup-tx-states.circom:39   */
    HZ_T_RQ_TX_VERIFIER = 12,  /* RqTxVerifier()                       src/rq-tx-verifier.circom:19     */
    HZ_T_MUX256 = 13,          /* Mux256()                             src/lib/mux256.circom:10         */
    HZ_T_BITS2AYSIGN = 14,     /* BitsCompressed2AySign()              src/lib/utils-bjj.circom:12      */
    HZ_T_AYSIGN2AX = 15,       /* AySign2Ax()                          src/lib/utils-bjj.circom:37      */
    /* circomlib 0.5.2's own sparse-Merkle-tree templates as main: the components behind src/rollup-tx.circom:537-570,
     * src/fee-tx.circom:97 (SMTProcessor(nLevels+1)) and src/withdraw.circom:47-58 (SMTVerifier(nLevels+1)). Here nLevels is the
     * template's own parameter (number of levels). Inputs as in circomlib: oldRoot, siblings[n], oldKey, oldValue, isOld0, newKey,
     * newValue, fnc[2] -> newRoot; enabled, root, siblings[n], oldKey, oldValue, isOld0, key, value, fnc. */
    HZ_T_SMT_PROCESSOR = 16,
    HZ_T_SMT_VERIFIER = 17,
    HZ_T_COUNT
} hz_template;

typedef struct {
    int32_t template_id; /* hz_template */
    int32_t nTx;         /* RollupMain / HashInputs only */
    int32_t nLevels;
    int32_t maxL1Tx;
    int32_t maxFeeTx;
    int32_t device;      /* HIP device ordinal */
    /* Number of independent instances of the main component evaluated by one hz_witness_run
     * (e.g. 2^20 Withdraw witnesses, or several RollupMain batches in flight). Inputs and the
     * witness carry the instance as the outermost index. 0 means 1. */
    int32_t n_instances;
    int32_t flags;       /* 0, or one of HZ_FLAG_* */
} hz_params;
/* HZ_FLAG_LATENCY: a RollupMain context of one to four batches puts its concurrent kernel chains -- front/hash/SMT/HashInputs, the
 * two signature kernels, the fee chain -- on disjoint sets of compute units through CU-masked streams: one 2048-transaction batch
 * alone 14.4 -> 7.7 ms (7.3 with HZ_FLAG_SOLO). Up to four such contexts in flight overlap (every context uses the same four masks): one batch each, 450 k
 * tx-witnesses/s with two, 640 k with four; plain contexts do not overlap in that regime (250 k). While at most TWO such contexts of one
 * batch are alive on the device their SMT chain kernel takes the latency form HZ_FLAG_SOLO describes (decided per launch; with four
 * in flight it would cost 15 %: profiles/r06_flagged_latency_form.txt). From eight batches per launch on,
 * the default (0 or HZ_FLAG_THROUGHPUT: any kernel on any CU) is faster. Every such context holds four hardware queues whose scratch
 * memory the runtime sizes by their hungriest kernel: within one process FOUR contexts per device get the partition by default
 * (HZ_MAX_PARTITIONED=<n> in the environment changes it; two until round 6, when a front kernel with 7.7 KB of scratch per lane made
 * four of them abort in the ROCm 7 runtime: profiles/r05_latency_regime.txt), further ones silently get the default schedule
 * (same witness). */
#define HZ_FLAG_THROUGHPUT 1
#define HZ_FLAG_LATENCY 2
/* HZ_FLAG_SOLO (with HZ_FLAG_LATENCY, contexts of ONE batch: no effect on larger ones): nothing else runs on the device while this context's step
 * does -- no second context in flight. Its SMT chain kernel then takes the latency form (a quad of lanes per chain, the level hash
 * spread over the quad: 0.67 x the chain's time for 2.5 x its instructions and a whole CU partition's wavefront slots -- which is why
 * it is wrong beside MANY other contexts: one batch x 4 contexts 540 k tx/s with it, 640 k without; a HZ_FLAG_LATENCY context takes it by
 * itself while at most two are alive; HZ_FLAG_SOLO keeps it whatever else exists). */
#define HZ_FLAG_SOLO 4

typedef struct {
    int32_t instance;      /* which instance failed */
    int32_t unit;          /* transaction / fee-tx index inside the instance, -1 if global */
    int32_t constraint_id; /* stable id, see hz_constraint_name() */
    uint8_t lhs[HZ_FR_BYTES];
    uint8_t rhs[HZ_FR_BYTES];
} hz_error;

typedef struct {
    const char* name; /* circom-style dotted name, e.g. main.rollupTx[3].processor1.newRoot */
    uint64_t index;   /* position in the flat witness of instance 0 */
} hz_symbol;

typedef struct hz_ctx hz_ctx;

/* library / device ----------------------------------------------------------------------- */
const char* hz_version(void);
const char* hz_last_error(void);          /* thread-local text of the last failure */
int32_t hz_device_count(void);            /* 0 when no gfx950 device is usable */

/* context: one compiled "circuit" ---------------------------------------------------------- */
hz_status hz_ctx_create(const hz_params* params, hz_ctx** out);
void hz_ctx_destroy(hz_ctx* ctx);
/* number of field elements in the witness of ONE instance (w[0] == 1 included) */
uint64_t hz_witness_len(const hz_ctx* ctx);
/* bytes of device memory the context holds, counting the buffers that are only allocated on first use (upload staging, the
 * signature ladder's side buffer of small launches): what n_instances of this template cost of a device's 288 GB */
uint64_t hz_ctx_device_bytes(const hz_ctx* ctx);
/* the same figure for a context that does not exist yet (no device needed): hz_template_device_bytes(&params) */
uint64_t hz_template_device_bytes(const hz_params* params);
/* closed-form constraint count of the template (reference tools/circuit-constraints.js:31-75) */
uint64_t hz_constraint_estimate(const hz_ctx* ctx);

/* inputs: `name` is a main-component input signal (e.g. "siblings1"); `vals` holds `count`
 * canonical 32-byte LE integers in circom's row-major flattening of the signal's dimensions,
 * for instance `instance`. For templates evaluated over n_instances, `instance` = -1 sets all
 * instances at once (`vals` = [n_instances][flat_len]). Values >= r are rejected. */
hz_status hz_set_input(hz_ctx* ctx, int32_t instance, const char* name, const uint8_t* vals, size_t count);
/* same layout and counts, but `dvals` already lives in device memory of ctx's device. NOTHING is range-checked on this route: the
 * caller guarantees canonical elements (< r), as the library's own *_dev outputs are; a witness computed from anything else means
 * nothing and no later call reports it. The CHECKED routes from device memory are hz_inputs_upload / hz_inputs_stage
 * (`packed` may be a device pointer): an element >= r there makes the next hz_witness_check answer HZ_ERR_INPUT. */
hz_status hz_set_input_dev(hz_ctx* ctx, int32_t instance, const char* name, const void* dvals, size_t count, void* stream);
/* forget which inputs were set (values are kept; calculateWitness semantics need a fresh set) */
/* Replicate all input signals of instance `src` onto instance `dst`, device to device, on `stream`.
 * (No reference counterpart: snarkjs computes one witness per call; this fills a multi-instance context.) */
hz_status hz_copy_instance_inputs(hz_ctx* ctx, int32_t src, int32_t dst, void* stream);
/* Forget which inputs were set (the next enqueue wants every one again) and whatever the library remembers of the buffer's content:
 * the step after it stores every signal, including the constants an earlier step left in place (DESIGN.md "constant marks"). */
void hz_clear_inputs(hz_ctx* ctx);
/* Bulk input path (the marshalling half of calculateWitness(input), reference test/helpers/helpers.js:147-149, for a process that
 * feeds batch after batch): ONE packed buffer per instance instead of one call per signal. Layout: every input signal in
 * hz_input_name order at hz_input_packed_offset(i) (32-byte aligned), as [outer][inner] little-endian elements -- the flattening
 * hz_set_input takes -- of hz_input_packed_width(i) bytes each: 32, or 1 for bit-valued signals (fromBjjCompressed).
 * hz_inputs_upload copies the buffer to the device asynchronously on `stream` (truly so from hz_host_alloc'ed pinned memory, which
 * the caller must keep unchanged until the stream reaches the copy) and one kernel scatters it into the witness layout and
 * range-checks the 32-byte elements; an element >= r is reported by the next hz_witness_check as HZ_ERR_INPUT.
 * `packed` may also be DEVICE memory (hz_inputs_upload / _stage / _stage_range alike): a host that keeps the packed inputs of its
 * batches resident in HBM hands each step's over with a device-to-device copy (bench.py's `value` loop). */
uint64_t hz_inputs_packed_bytes(const hz_ctx* ctx);
int32_t hz_input_packed_width(const hz_ctx* ctx, int32_t i);
uint64_t hz_input_packed_offset(const hz_ctx* ctx, int32_t i);
void* hz_host_alloc(size_t bytes);
void hz_host_free(void* p);
hz_status hz_inputs_upload(hz_ctx* ctx, int32_t instance, const void* packed, size_t bytes, void* stream);
/* The copy alone, ahead of time: the packed buffer goes to the instance's device staging slot on `stream` (NULL = the context's
 * copy stream) and the NEXT hz_witness_enqueue / hz_witness_run scatters every staged instance into the witness layout before
 * its kernels. Called right after the enqueue of step N with the inputs of step N + 1, the PCIe transfer overlaps step N's
 * kernels, which still read the old inputs. All stage calls between two enqueues of a context must use the same stream. */
hz_status hz_inputs_stage(hz_ctx* ctx, int32_t instance, const void* packed, size_t bytes, void* stream);
/* The same for `count` consecutive instances, instance first + j from packed + j * stride. When the host buffers are contiguous
 * (stride == bytes_each) the whole range crosses PCIe as one copy: what a serving loop calls once per step. */
hz_status hz_inputs_stage_range(hz_ctx* ctx, int32_t first, int32_t count, const void* packed, size_t bytes_each, size_t stride, void* stream);
/* enumerate the input signals the template expects */
int32_t hz_input_count(const hz_ctx* ctx);
const char* hz_input_name(const hz_ctx* ctx, int32_t i, uint64_t* flat_len);

/* run: all instances, inputs resident in HBM. Asynchronous variant enqueues on `stream` and
 * returns; hz_witness_check then synchronises and reports the first violated constraint
 * (lowest instance, lowest unit, lowest constraint id). hz_witness_run = enqueue + check. */
hz_status hz_witness_enqueue(hz_ctx* ctx, void* stream);
hz_status hz_witness_check(hz_ctx* ctx, hz_error* err);
hz_status hz_witness_run(hz_ctx* ctx, hz_error* err);
/* After hz_witness_check / hz_witness_run: the first violated constraint of EVERY instance of that launch, ordered by instance
 * (out[0] is what hz_witness_check reported). The reference evaluates one circuit per calculateWitness call and throws at its first
 * failing `===` (test/rollup-main.test.js:868-877, test/rollup-tx.test.js:911-918); a launch here evaluates n_instances of them, and
 * a serving loop has to know every batch to reject, not only the first. *n_failed = number of failing instances (0 when the launch
 * was clean), of which min(cap, *n_failed) are written. cap = 0 only counts; otherwise the operands cost one more pass over the
 * kernels when there are failures. */
hz_status hz_witness_failures(hz_ctx* ctx, hz_error* out, size_t cap, size_t* n_failed);

/* Per-kernel timing of the last enqueue, measured with HIP events on the launch stream.
 * `algorithmic_bytes` = 32 B x (witness signals the kernel is responsible for) x units.
 * on = 1: the normal schedule (EdDSA and fee chains overlap the hash/SMT chain on side streams);
 * on = 2: exclusive, every kernel alone on the device (durations usable for a per-kernel roofline). */
hz_status hz_ctx_set_profiling(hz_ctx* ctx, int32_t on);
int32_t hz_profile_count(const hz_ctx* ctx);
hz_status hz_profile_get(hz_ctx* ctx, int32_t i, const char** kernel, float* ms, uint64_t* algorithmic_bytes, uint64_t* units);

/* output: copy `count` elements starting at flat index `first` of instance `instance` to host */
hz_status hz_witness_read(hz_ctx* ctx, int32_t instance, uint64_t first, uint64_t count, uint8_t* out);
/* The physical buffer: sections stored signal-major (include/hz_layout.h); `total` elements. For
 * instanced templates element (signal s, instance k) sits at s * n_instances + k. */
uint64_t hz_witness_total(const hz_ctx* ctx);
hz_status hz_witness_read_raw(hz_ctx* ctx, uint64_t first, uint64_t count, uint8_t* out);
const void* hz_witness_dev_ptr(const hz_ctx* ctx);

/* wire / disk formats ------------------------------------------------------------
 * hz_set_inputs_json: the input.json the reference's tools write (tools/generate-input.js:109; decimal strings, bare
 *   integers, 0x-hex, nested arrays; values reduced mod r) -> hz_set_input per key.
 * hz_witness_write_json: witness.json, array of decimal strings (tools/helpers/actions.js:136-139).
 * hz_witness_write_wtns: snarkjs .wtns (version 2: header section {n8 = 32, prime, nVars}, data section nVars x 32 B LE).
 * hz_symbols_write_sym: circom .sym lines `labelIdx,varIdx,componentIdx,name` for the stored signals. */
hz_status hz_set_inputs_json(hz_ctx* ctx, int32_t instance, const char* json, size_t len);
hz_status hz_witness_write_json(hz_ctx* ctx, int32_t instance, const char* path);
hz_status hz_witness_write_wtns(hz_ctx* ctx, int32_t instance, const char* path);
hz_status hz_symbols_write_sym(const hz_ctx* ctx, const char* path);

/* circom .sym import: the witness in the COMPILER's variable order. The reference's prover steps (snarkjs / rapidsnark on the
 * r1cs + zkey of tools/helpers/actions.js:30-68,148-170) consume circom's numbering, which only the compiler's .sym records
 * (`labelIdx,varIdx,componentIdx,name`; varIdx = -1 for eliminated signals; wired labels share a varIdx). hz_symmap_create joins
 * it by name with the signals this library stores: a variable resolves when any of its labels is stored. hz_symmap_unresolved
 * returns how many variables did not (and the i-th one's number and a label): a compile that keeps signals this layout drops
 * cannot be served. hz_witness_read_sym / hz_witness_write_wtns_sym then deliver the witness in that order;
 * hz_witness_gather reads arbitrary positions of this library's own per-instance numbering. */
typedef struct hz_symmap hz_symmap;
hz_status hz_symmap_create(const hz_ctx* ctx, const char* sym_text, size_t len, hz_symmap** out);
void hz_symmap_destroy(hz_symmap* map);
uint64_t hz_symmap_nvars(const hz_symmap* map);
uint64_t hz_symmap_unresolved(const hz_symmap* map, uint64_t i, uint64_t* var, const char** name);
/* how many variables of the map are DERIVED: linear signals this layout does not store and a compile without constraint reduction
 * keeps (reference test/rollup-main.test.js:52, reduceConstraints:false) -- every signal inside a Poseidon component (ark / mix /
 * S-box inputs, from the stored S-box products), and the linear intermediates / linearly fed component inputs of the reference's own
 * templates (rule table in csrc/formats.hip) -- evaluated from stored signals when the witness is read in the compiler's order */
uint64_t hz_symmap_derived(const hz_symmap* map);
/* .sym AND .r1cs of the same compile (tools/helpers/actions.js:30-68 writes both). Variables that no label resolves -- the
 * wire-through signals an unreduced compile keeps: inputs of sub-components, aliases of their outputs, Bits2Num sums, comparator
 * differences, for ANY circuit and circomlib version -- are solved from the circuit's own LINEAR constraints: one with exactly one
 * unknown variable defines it over known ones, and so on until nothing changes (hz_symmap_solved = how many); a product constraint
 * A * B = C whose A and B are known and whose C holds one unknown variable defines that one too (a product signal the layout does
 * not store under that name, e.g. MultiMux4's terms over constant inputs). The r1cs stays with
 * the map: hz_symmap_check_r1cs evaluates every constraint (A.w)(B.w) = C.w on the witness as the map serves it -- what
 * `snarkjs wtns check` would do with the .wtns this library writes -- and returns the number of violated constraints and the
 * indices of the first `cap` of them. r1cs: iden3 binary format version 1, field BN254 Fr; circom's wire w is variable w. */
hz_status hz_symmap_create_r1cs(const hz_ctx* ctx, const char* sym_text, size_t sym_len, const uint8_t* r1cs, size_t r1cs_len, hz_symmap** out);
uint64_t hz_symmap_solved(const hz_symmap* map);
hz_status hz_symmap_check_r1cs(hz_ctx* ctx, const hz_symmap* map, int32_t instance, uint64_t* n_bad, uint64_t* first_bad, uint64_t cap);
/* A resolved map on disk: importing the files of a full-size circuit takes minutes, the map is a few arrays. A map belongs to one
 * template and shape (checked on load); the constraint system is not kept (hz_symmap_check_r1cs needs a map made from the files). */
hz_status hz_symmap_save(const hz_ctx* ctx, const hz_symmap* map, const char* path);
hz_status hz_symmap_load(const hz_ctx* ctx, const char* path, hz_symmap** out);
hz_status hz_witness_read_sym(hz_ctx* ctx, const hz_symmap* map, int32_t instance, uint64_t first_var, uint64_t count, uint8_t* out);
hz_status hz_witness_write_wtns_sym(hz_ctx* ctx, const hz_symmap* map, int32_t instance, const char* path);
hz_status hz_witness_gather(hz_ctx* ctx, int32_t instance, const uint64_t* index, uint64_t count, uint8_t* out);

/* The witness in the compiler's order ON THE DEVICE (SURVEY 8a' K8): what a prover on the same GPU consumes. The reference hands
 * w[] over in circom's numbering (test/helpers/helpers.js:142,149) and its prove step reads that vector beside the .r1cs / zkey
 * (tools/helpers/actions.js:132-170); the kernels of a step write a signal-major layout of their own (include/hz_layout.h).
 *   hz_symmap_upload            takes the map to the context's device once (the first export does it implicitly): per 128-byte line of
 *                               the physical buffer -- four consecutive units of one signal -- the four variables it feeds, ordered
 *                               so that consecutive lanes write consecutive variables; CSR tables of the derived variables.
 *                               device_bytes (optional) = size of those tables.
 *   hz_witness_export_dev       ONE pass: variable v of instance `instance` -> d_out[v] (hz_symmap_nvars x 32 bytes, canonical LE),
 *                               stored variables gathered, derived ones (an unreduced compile's linear signals) evaluated on the
 *                               device. instance = -1: every instance, d_out[instance][v]. Asynchronous on `stream` (NULL = the
 *                               context's stream), ordered after a hz_witness_enqueue on the same stream.
 *   hz_witness_export_range_dev the same for instances [first, first + count)
 *   hz_witness_export_host      the same pass, then asynchronous copies through a ring of two pinned buffers into `out`
 *                               (count x 32 bytes from variable first_var on); PCIe bound: 3.86 GB per headline batch at <= 63 GB/s.
 *                               hz_witness_write_wtns_sym and hz_symmap_check_r1cs run on exactly this buffer.
 *   hz_symmap_dev_index         for a consumer that prefers indirection over a copy: phys0[v] = element of hz_witness_dev_ptr() that
 *                               holds variable v of instance 0, inst_stride[v] = elements to add per instance; a derived variable
 *                               has phys0[v] = 2^63 | k, its value is element (instance slot) * n_derived_slots + k of the buffer
 *                               hz_witness_derive_dev fills (instance = -1: slot = instance; otherwise slot 0). */
/* A map given explicitly -- variable v is signal index[v] of this library's per-instance numbering, variable 0 the constant --
 * and the stored signals in component-major order (every unit's signals together: the shape of a reducing compile's numbering)
 * as such an index: hz_component_major_index returns the number of entries and writes min(cap, that). */
hz_status hz_symmap_from_index(const hz_ctx* ctx, const uint64_t* index, uint64_t n, hz_symmap** out);
uint64_t hz_component_major_index(const hz_ctx* ctx, uint64_t* index, uint64_t cap);
hz_status hz_symmap_upload(hz_ctx* ctx, const hz_symmap* map, uint64_t* device_bytes);
hz_status hz_witness_export_dev(hz_ctx* ctx, const hz_symmap* map, int32_t instance, void* d_out, void* stream);
hz_status hz_witness_export_range_dev(hz_ctx* ctx, const hz_symmap* map, int32_t first_instance, int32_t count, void* d_out, void* stream);
hz_status hz_witness_export_host(hz_ctx* ctx, const hz_symmap* map, int32_t instance, uint64_t first_var, uint64_t count, uint8_t* out);
hz_status hz_symmap_dev_index(hz_ctx* ctx, const hz_symmap* map, const uint64_t** d_phys0, const uint32_t** d_inst_stride, uint64_t* n_derived_slots);
hz_status hz_witness_derive_dev(hz_ctx* ctx, const hz_symmap* map, int32_t instance, const void** d_derived, void* stream);

/* symbols ------------------------------------------------------------------------------------ */
uint64_t hz_symbol_count(const hz_ctx* ctx);
hz_status hz_symbol_get(const hz_ctx* ctx, uint64_t i, hz_symbol* out);
/* returns 1 and the index if `name` (with or without the "main." prefix) is a witness signal */
int32_t hz_symbol_lookup(const hz_ctx* ctx, const char* name, uint64_t* index);
const char* hz_constraint_name(int32_t constraint_id);

/* Evaluates a DAG of Poseidon hashes on the device, level by level: the Merkle work of a batch builder (the counterpart of
 * @hermeznetwork/commonjs RollupDB / BatchBuilder, called by the reference at test/helpers/helpers.js:46,148 and
 * tools/generate-input.js:70-107, which hashes 2*(nLevels+1) dependent nodes per transaction on one CPU thread).
 * `vals` is a table of n_vals field elements (32-byte little-endian, canonical) in host memory: known values on entry, every
 * job's digest on return. Job j hashes the seg_t-1 elements vals[job_in[6*j + k]] and stores Poseidon(seg_t) at vals[job_out[j]].
 * Jobs are listed in execution order in segments [seg_first, seg_first+seg_count) of one width seg_t (2..7); the jobs of a segment
 * must not depend on each other (all node versions of one tree level form one segment). device_ms (optional) receives the
 * device time of the segment launches. */
#define HZ_DAG_MAX_IN 6
hz_status hz_poseidon_dag(int32_t device, uint8_t* vals, uint64_t n_vals, const uint32_t* job_in, const uint32_t* job_out, uint64_t n_jobs,
                          const uint32_t* seg_t, const uint64_t* seg_first, const uint64_t* seg_count, uint32_t n_segs, double* device_ms);

/* Device-resident account tree: the pre-populated state of a rollup kept, updated and proven in HBM (the role RollupDB's state tree
 * plays behind @hermeznetwork/commonjs BatchBuilder, reference test/helpers/helpers.js:46,148; leaf = src/lib/hash-state.circom:14-40).
 * An hz_state is a perfect binary tree of depth k over the N = 2^k consecutive accounts first_idx .. first_idx + N - 1, the geometry of
 * circuits_amd/builder.py DenseState: node (d, p) covers the keys = p (mod 2^d), its children are (d + 1, p) and (d + 1, p + 2^d),
 * leaves sit at depth k, key bits LSB first as in circomlib. The k + 1 level arrays and the N state hashes stay on the device.
 *   hz_state_create / _destroy   4 <= k <= 24; a failed allocation is HZ_ERR_HIP with the runtime's text in hz_last_error
 *   hz_state_load       builds the whole tree on the device from four host arrays of [N][32] leaf fields (e0 = tokenID + nonce * 2^32 +
 *                       sign * 2^72, balance, ay, ethAddr), indexed by account j = idx - first_idx: state hash Poseidon(5), leaf hash
 *                       Poseidon(4) of (idx, state hash, 1), k levels of Poseidon(3): one upload, k + 2 launches, no level returns to the host
 *   hz_state_root       the current root
 *   hz_state_apply      m ORDERED updates of EXISTING accounts (m <= 65536; idx[m], fields[m][4][32] as above), sequential semantics: update j
 *                       sees the tree as updates 0 .. j - 1 left it; an account may appear any number of times. Outputs in host memory,
 *                       each may be NULL: siblings_out [m][n_sib][32] (root side first, zero beyond depth k; n_sib >= k, the circuits
 *                       want nLevels + 1), old_value_out [m][32] (the leaf's state hash before update j), old_root_out / new_root_out
 *                       [m][32] (the root before / after update j): with oldKey = newKey = idx and fnc = (0, 1) the inputs of
 *                       circomlib's SMTProcessor. The tree is updated in place; the next call sees the consolidated state. An idx outside
 *                       the state is HZ_ERR_ARG and leaves the tree untouched. The dependent work is k + 2 launches whatever m is (node
 *                       versions, DESIGN.md "Device-resident account tree").
 *   hz_state_proofs     membership proofs against the current root (SMTVerifier's inputs): siblings_out [n][n_sib][32], value_out
 *                       [n][32] state hashes; a gather on the device
 *   hz_state_download   the arrays in DenseState's layout: levels_out[d] receives the 2^d digests of level d (d = 0 .. k; a NULL entry is
 *                       skipped), value_out the N state hashes -- what hzb_db_set_base (hz_host.h) takes as a base
 *   hz_state_device_ms  device time of the last load / apply (first kernel to write-back, HIP events)
 * OUT OF SCOPE: inserts and new accounts (a deposit that creates a leaf changes the tree's shape), the exit tree, transaction semantics
 * (balances, nonces, fees: hz_ledger's, below), more than one device per state. A state is used by one thread at a time. */
typedef struct hz_state hz_state;
hz_status hz_state_create(int32_t device, int32_t k, uint64_t first_idx, hz_state** out);
void hz_state_destroy(hz_state* st);
hz_status hz_state_load(hz_state* st, const uint8_t* e0, const uint8_t* balance, const uint8_t* ay, const uint8_t* eth_addr);
hz_status hz_state_root(hz_state* st, uint8_t* out32);
hz_status hz_state_apply(hz_state* st, size_t m, const uint64_t* idx, const uint8_t* fields, size_t n_sib, uint8_t* siblings_out,
                         uint8_t* old_value_out, uint8_t* old_root_out, uint8_t* new_root_out);
hz_status hz_state_proofs(hz_state* st, size_t n, const uint64_t* idx, size_t n_sib, uint8_t* siblings_out, uint8_t* value_out);
hz_status hz_state_download(hz_state* st, uint8_t* const* levels_out, uint8_t* value_out);
double hz_state_device_ms(const hz_state* st);

/* Sparse device-resident Merkle tree: a circomlib SMT in HBM that accepts INSERTS as well as updates -- the exit tree of a batch (empty at
 * its start, filled by inserts and updates), the state tree under create-account deposits (idx = lastIdx + 1), membership proofs for
 * Withdraw. Keys are below 2^48, bits LSB first; the value of a leaf is the state hash Poseidon(5) of its four fields (e0, balance, ay,
 * ethAddr, as hz_state_load), its hash Poseidon(4) of (key, value, 1). The digests live in device pools that grow on demand; the host
 * keeps the shape as integers (no field arithmetic and no hash there), DESIGN.md 8b.
 *   hz_smt_create / _destroy   an empty tree; n_sib_max (1 .. 64) bounds the n_sib of later calls. A failed allocation, here or when a
 *                       pool grows, is HZ_ERR_HIP
 *   hz_smt_reset        the empty tree again, pools kept: the exit tree of the next batch
 *   hz_smt_root / _size the current root (0 for the empty tree); the number of keys held
 *   hz_smt_apply        m ORDERED operations (m <= 65536; key[m], fields[m][4][32]) with sequential semantics: operation j inserts its key
 *                       when the tree as operations 0 .. j - 1 left it does not hold it, and updates it otherwise. Outputs in host
 *                       memory, each may be NULL, are the inputs of circomlib's SMTProcessor(n_sib) for operation j with newKey = key[j]
 *                       and newValue = the state hash: siblings_out [m][n_sib][32] (root side first, zero-padded), old_key_out [m],
 *                       old_value_out [m][32], is_old0_out [m] (an insert into an empty slot: old key = key, old value 0; an insert
 *                       that meets another leaf reports that leaf's key and value; an update its own key and previous value),
 *                       fnc_out [m] (0 update: fnc = [0, 1]; 1 insert: fnc = [1, 0]), old_root_out / new_root_out [m][32]. The
 *                       dependent device work is max depth + 2 launches whatever m is
 *   hz_smt_proofs       proofs against the current root (SMTVerifier's inputs, fnc 0 where found_out[i] and fnc 1 otherwise):
 *                       siblings_out [n][n_sib][32], value_out [n][32] (found keys), not_found_key_out [n] / not_found_value_out [n][32]
 *                       / is_old0_out [n] (absent keys: the leaf the lookup met, or the key itself, 0 and is_old0 = 1 at an empty slot);
 *                       n <= 2^20; a gather on the device
 *   hz_smt_plan         DIAGNOSTIC: the host planner alone on an empty tree -- integers only, works without a device: the depth of each
 *                       operation's leaf, fnc, old key and is_old0 as hz_smt_apply would report them
 *   hz_smt_device_ms    device time of the last apply (first kernel to write-back, HIP events)
 * A failing call names the offending operation in hz_last_error and leaves the tree untouched: root, size and later results are as if
 * it had not been made; a refused hz_smt_proofs writes to none of its outputs. The one exception is a HIP failure reported AFTER a
 * call's write-back was queued (the copies out, the final synchronise): the pools may then hold part of that call, so the shape is
 * rolled back and every later apply / proofs / root answers HZ_ERR_HIP until hz_smt_reset. No failing call leaves work in flight. HZ_ERR_ARG: null arguments, m over the cap, n_sib outside 1 .. 64 or above n_sib_max. HZ_ERR_INPUT: a key >=
 * 2^48, a field >= r, an operation whose leaf would sit at depth >= n_sib (an insert SMTProcessor(n_sib) cannot express; a proof that
 * needs n_sib or more siblings likewise).
 * OUT OF SCOPE: transaction semantics, deletes (Hermez never deletes), more than one device per tree. One thread at a time. */
typedef struct hz_smt hz_smt;
hz_status hz_smt_create(int32_t device, int32_t n_sib_max, hz_smt** out);
void hz_smt_destroy(hz_smt* t);
hz_status hz_smt_reset(hz_smt* t);
hz_status hz_smt_root(hz_smt* t, uint8_t* out32);
uint64_t hz_smt_size(const hz_smt* t);
double hz_smt_device_ms(const hz_smt* t);
hz_status hz_smt_apply(hz_smt* t, size_t m, const uint64_t* key, const uint8_t* fields, size_t n_sib, uint8_t* siblings_out, uint64_t* old_key_out,
                       uint8_t* old_value_out, uint8_t* is_old0_out, uint8_t* fnc_out, uint8_t* old_root_out, uint8_t* new_root_out);
hz_status hz_smt_proofs(hz_smt* t, size_t n, const uint64_t* key, size_t n_sib, uint8_t* siblings_out, uint8_t* found_out, uint8_t* value_out,
                        uint64_t* not_found_key_out, uint8_t* not_found_value_out, uint8_t* is_old0_out);
hz_status hz_smt_plan(size_t m, const uint64_t* key, size_t n_sib, uint32_t* depth_out, uint8_t* fnc_out, uint64_t* old_key_out, uint8_t* is_old0_out);

/* Device-resident ledger: an hz_state plus the four leaf-field planes (e0, balance, ay, ethAddr; [N][32] each) kept in HBM, so that a
 * batch of L2 transfers between existing accounts -- and the fee transactions that end it -- is computed AND applied on the device: the
 * amounts (float40), fees (src/compute-fee.circom), balances and nonces with the sequential semantics of BatchBuilder.build in
 * circuits_amd/builder.py (its L2 branch is the checker), then the tree update of hz_state_apply on the new leaves, without a host
 * round trip for any 256-bit value. The outputs are every state-dependent input RollupMain wants for such a batch.
 *   hz_ledger_create / _destroy   as hz_state_create (4 <= k <= 24)
 *   hz_ledger_load      as hz_state_load, but the planes stay resident. The planes must be LEAVES: balance < 2^192, e0 < 2^73 (tokenID |
 *                       nonce << 32 | sign << 72), ethAddr < 2^160 -- every kernel assumes it. Anything else is HZ_ERR_INPUT with the
 *                       first offending account named, before the tree or the planes are touched: a ledger that was loaded before
 *                       keeps its root and fields
 *   hz_ledger_root      the current root
 *   hz_ledger_accounts  the resident leaf fields of n accounts: fields_out [n][4][32]
 *   hz_ledger_tree      the tree, borrowed: hz_state_proofs / _download / _root work on it (hz_state_apply / _load on it would leave the
 *                       planes behind: do not)
 *   hz_ledger_apply_l2  m ordered transactions and F fee slots (F <= 64; fee_plan_tokens[F] zero-padded as feePlanTokens is,
 *                       fee_idxs[F] with 0 = unused slot). from_idx == 0 is a NOP (padding). Transaction i, in order: amount =
 *                       float2fix(amount_f); fee = amount * table[user_fee] >> 60 below selector 192, amount * table[user_fee] from 192
 *                       on; the sender's balance -= amount + fee, nonce += 1; when amount != 0 the receiver -- as it stands after the
 *                       sender's update: a self-transfer sees the new leaf -- gets balance += amount, otherwise processor 2 is a NOP
 *                       (its fields zero except tokenID2 = token_id, siblings2 zero, no update). The fee is added to the first slot s
 *                       with fee_plan_tokens[s] == token_id (padding zeros included, as plan.index does), to none if no slot matches.
 *                       After the last transaction slot j with fee_idxs[j] != 0 adds accumulated fee j to that account, in slot order.
 *                       The updates of a call (two per active transaction, minus receivers of zero amounts, plus active fee slots) must
 *                       be at most 65536; k <= n_sib <= 64 (the circuits want nLevels + 1). `out` (may be NULL) is a struct of nullable
 *                       host pointers; every array is canonical 32-byte little-endian elements in the row-major flattening
 *                       hz_set_input takes.
 *   hz_ledger_outputs_dev  the same arrays as DEVICE pointers of the last successful apply, valid until the ledger's next call: each can
 *                       go to hz_set_input_dev unchanged
 *   hz_ledger_plan_l2   DIAGNOSTIC, no device: the integer plan alone. Events are the updates in order (sender, then receiver, of each
 *                       transaction; then the fee slots). Per transaction: ev_sender_out / ev_receiver_out (event number or -1),
 *                       fee_slot_out (or -1), last_event_out (last event of transactions 0 .. i, -1 none). Per event (room for
 *                       2 m + F): ev_account_out, ev_prev_out (the previous event on the same account or -1). Every output may be NULL
 *   hz_ledger_device_ms / _semantic_ms  device time of the last apply: first kernel to the last write-back; first kernel to the
 *                       failure-word read (the semantic kernels alone)
 * REFUSALS. A batch the circuit would reject is refused as a whole with HZ_ERR_INPUT; hz_last_error names the LOWEST offending
 * transaction index and one reason, the lowest reason code if several hold there:
 *   1 the sender's token != token_id          2 nonce != the sender's current nonce      3 the sender's balance < amount + fee
 *   4 the receiver's token != token_id (only when amount != 0)       5 a new balance >= 2^192
 *   6 fee slot j: the account's token != fee_plan_tokens[j], reported with index m + j, after every transaction
 *   12 the sender's nonce is 2^40 - 1: the next nonce is not a leaf field. The circuit does not wrap (src/rollup-tx.circom:519 feeds
 *      nonce + 1 into the state hash), so neither does the ledger. It ranks like 1 - 8 (lowest index, then lowest reason) in every call
 *      that applies L2 transactions. A transaction nonce of 2^40 or more never equals a resident nonce: that is reason 2
 *   16 (HZ_LEDGER_FEE_OVERFLOW) amount x fee factor does not fit 128 bits (src/compute-fee.circom:89-91): the fee, amount * table[user_fee]
 *      after the shift, is 2^128 or more. Selectors 31 to 255 can reach it with a float40 amount, selectors 0 to 30 cannot. Checked only
 *      where the circuit applies the fee: an L2 row that is not a NOP, exits included; an L1 row and a NOP are never refused for it. It
 *      ranks with 1 - 8, 12 and 13 (lowest row, then lowest reason; reason 9 keeps its precedence) in all seven apply calls
 * builder.py raises for 1, 3 and 6 and builds inputs the circuit rejects for 2 and 4; the ledger refuses those two as well.
 * builder.py also builds inputs the circuit rejects for 16, as upstream's BatchBuilder does; the ledger refuses them. A refused
 * call changes nothing (fields, tree, root), writes none of its outputs and leaves no work in flight; the one exception is hz_smt_apply's:
 * a HIP failure reported after the write-back was queued. HZ_ERR_ARG: null arguments, an index outside the state, to_idx 0 or 1 (transfer
 * to an address, exit: not supported yet), amount_f >= 2^40, too many updates, n_sib outside k .. 64, F > 64, apply before load.
 * SIGNATURES. hz_ledger_apply_l2 looks at no signature; the calls below verify every L2 signature on the device, against
 * the sender's RESIDENT key (ay, sign), before anything is applied:
 *   hz_ledger_apply_l2_signed  hz_ledger_apply_l2 with sigs[m] (entry i belongs to txs[i]; a NOP's entry is ignored) and the checks of
 *                       EdDSAPoseidonVerifier and of maxNumBatch added. The message is M = Poseidon(6)(txCompressedData, toEthAddr |
 *                       amountF << 160 | maxNumBatch << 200, toBjjAy, 0, 0, 0) (src/decode-tx.circom:249-283, rq* fields zero). Accepted
 *                       iff S < l, AySign2Ax finds Ax for the resident (ay, sign), 8 A has x != 0, and BabyAdd(R8, hm * 8A) == S * B8
 *                       with hm = Poseidon(5)(R8x, R8y, Ax, Ay, M) as the full integer, the affine formula on R8 as given (R8 is not
 *                       checked to be on the curve) and both of its denominators nonzero. sig_out (may be NULL; nullable host
 *                       pointers): txCompressedData, txCompressedDataV2 and M of every transaction, [m] each; a NOP's rows are those of
 *                       the empty transaction
 *   hz_ledger_verify_l2 the mempool filter: the same kernels, one verdict per transaction (0 accepted or NOP, 7, 8; 7 beside 8 is 7) in
 *                       verdict_out[m]. Changes nothing resident and refuses nothing; the transactions need not be applicable in order.
 *                       It and hz_ledger_verify_l2_atomic are signature and link filters (0, 7, 8, 13): neither knows reason 16
 *   hz_ledger_sig_outputs_dev  sig_out's arrays as DEVICE pointers of the last successful hz_ledger_apply_l2_signed / _verify_l2, valid
 *                       until the ledger's next call; fit for hz_set_input_dev
 *   hz_ledger_sig_ms    device time of the two signature kernels of the last such call
 * Further refusal reasons of hz_ledger_apply_l2_signed, in the same order with reasons 1 - 6 (lowest index, then lowest reason):
 *   7 the signature is rejected (any cause above)       8 max_num_batch != 0 and max_num_batch < current_num_batch
 * HZ_ERR_INPUT: s, r8x, r8y or to_bjj_ay >= r. HZ_ERR_ARG: null sigs, to_eth_addr >= 2^160, chain_id >= 2^16, to_bjj_sign > 1, and
 * everything hz_ledger_apply_l2 refuses as an argument.
 * RECEIVERS BY ADDRESS OR KEY. A transaction with to_idx == 0 is transferToEthAddr / transferToBjj: the user signs
 * to_eth_addr, or the "any" address 2^160 - 1 plus (to_bjj_ay, to_bjj_sign), and the coordinator picks the receiver. The four calls above
 * keep refusing it; these accept it:
 *   hz_ledger_apply_l2_addr  hz_ledger_apply_l2 over transactions whose to_idx may be 0. sigs[m] is required: its destination fields are
 *                       always read; s, r8x, r8y only with HZ_LEDGER_VERIFY_SIGS in flags, and the call then verifies exactly as
 *                       hz_ledger_apply_l2_signed does (reasons 7 and 8; sig_out as there). Without the flag sig_out must be NULL and
 *                       chain_id / current_num_batch are not looked at. For an active transaction with to_idx == 0 and amount != 0 the
 *                       receiver is aux_to_idx[i] when that array is given (the entry must lie inside the state), and otherwise the
 *                       LOWEST index whose leaf holds to_eth_addr -- or, when to_eth_addr is the "any" address, that address with ay ==
 *                       to_bjj_ay and sign == to_bjj_sign -- and the token token_id, found on the device in the resident planes as they
 *                       are before the batch (keys, addresses and tokens never change in an L2 batch, so that is exact). The receiver
 *                       then behaves as in a plain transfer: it sees the sender's update, and a transfer to one's own address that
 *                       resolves to the sender sees the new leaf. With amount == 0 processor 2 is a NOP, nothing is looked up, and the
 *                       leaf-2 rows are what the circuit compares with the signed destination: ethAddr2 = to_eth_addr and, under the
 *                       "any" address, ay2 = to_bjj_ay and sign2 = to_bjj_sign; tokenID2 = token_id, the rest zero, siblings2 zero.
 *                       to_idx >= 2 is today's transfer; to_idx == 1 stays HZ_ERR_ARG. The signed to_idx (0) is what txCompressedData,
 *                       txCompressedDataV2 and the message carry. aux_to_idx_out (may be NULL): auxToIdx as [m][32] elements -- the
 *                       receiver of a to_idx == 0 transaction with amount != 0, otherwise 0.
 *   hz_ledger_resolve_l2  the lookup alone: aux_to_idx_out[m], 0 for a NOP, for to_idx != 0 or when nothing matches; a zero amount is
 *                       still resolved. Changes nothing and refuses nothing.
 *   hz_ledger_aux_to_idx_dev  the auxToIdx rows as a DEVICE pointer, [m][32] of the last successful hz_ledger_apply_l2_addr, valid until
 *                       the ledger's next call; fit for hz_set_input_dev
 *   hz_ledger_resolve_ms  device time of the two lookup kernels of the last hz_ledger_apply_l2_addr / _resolve_l2 (0: none ran)
 * Further refusal reasons of hz_ledger_apply_l2_addr:
 *   9 no account holds the signed destination with the transaction's token. The lookup runs before the plan of the batch can exist, so
 *     reason 9 is reported FIRST: it names the lowest such transaction whatever else is wrong with the batch (a lower transaction with a
 *     reason of 1 - 8 included).
 *   10 the receiver's ethAddr != to_eth_addr     11 under the "any" address: the receiver's ay / sign != to_bjj_ay / to_bjj_sign
 *   10 and 11 are reachable only through a supplied aux_to_idx and rank with 1 - 8: lowest index, then lowest reason.
 * L1 TRANSACTIONS. A batch RollupMain proves is a run of L1 transactions followed by L2 transactions; the calls above take
 * the L2 part alone. An hz_l1tx is a deposit, depositTransfer or forceTransfer on EXISTING accounts: from_idx != 0, to_idx 0 (no transfer)
 * or >= 2, amount_f and load_amount_f float40, token_id, from_eth_addr as 32 little-endian bytes below 2^160. An invalid L1 transaction
 * is not refused, it is NULLIFIED (src/rollup-tx-states.circom:244-313, src/balance-updater.circom:56-100; the onChain branch of
 * BatchBuilder.build is the checker). From the leaves as they are before the batch:
 *   null_tok1 = token_id != sender.tokenID          null_load = null_tok1 && loadAmount != 0
 *   null_eth  = amount != 0 && from_eth_addr != sender.ethAddr     null_tok2 = amount != 0 && token_id != receiver.tokenID
 *   null_amount = null_eth || null_tok2 || (null_tok1 && amount != 0)
 * and then, in order over the L1 transactions, on the balances as the earlier ones left them:
 *   eff_load = null_load ? 0 : loadAmount           eff2 = null_amount ? 0 : amount
 *   underflow_ok = balance[sender] + eff_load - eff2 >= 0          eff3 = underflow_ok ? eff2 : 0
 *   balance[sender] += eff_load - eff3, then balance[receiver] += eff3 (a self-transfer sees the sender's new leaf)
 *   isAmountNullified = !(!null_amount && underflow_ok)
 * No fee, no nonce check or increment, no signature. Whenever amount != 0 (the float40's mantissa is not zero), nullified or not,
 * processor 2 is an UPDATE of the receiver with delta eff3: its before-leaf and siblings are written; with amount == 0 it is a NOP and
 * all six leaf-2 rows are zero (tokenID2 too). So what a receiver gets depends on its sender's balance at that moment, which depends on
 * whether earlier transfers into that sender were nullified: the device walks the L1 run in order over balances held in LDS.
 *   hz_ledger_apply_batch  n_l1 L1 transactions (n_l1 <= HZ_LEDGER_MAX_L1), then m L2 transactions exactly as hz_ledger_apply_l2_addr
 *                       takes them (flags, aux_to_idx[m], sig_out[m] belong to the L2 rows; sigs may be NULL when
 *                       HZ_LEDGER_VERIFY_SIGS is not set and no L2 transaction has to_idx == 0). The batch has n_l1 + m rows, L1 first:
 *                       every [m] array of `out` has n_l1 + m rows, acc_fee_after rows of the L1 run are zero, aux_to_idx_out is
 *                       [n_l1 + m][32] with zero L1 rows. l1_flags_out (may be NULL): one byte per L1 transaction, bit 0
 *                       nullifyLoadAmount, bit 1 isAmountNullified. Refusals name the ROW (n_l1 + i for L2 transaction i). Reasons 1 - 4
 *                       never fire for an L1 row; reason 5 can, through loadAmount, and stays a refusal (the circuit's Num2Bits(193)
 *                       rejects it). An L2 transaction funded by an L1 deposit is accepted; one that counted on a nullified L1 transfer
 *                       is refused with reason 3 at its own row. Reason 9 keeps its precedence. With n_l1 == 0 every output equals
 *                       hz_ledger_apply_l2_addr's byte for byte. HZ_ERR_ARG beyond that call's: L1 from_idx == 0 (creates an
 *                       account), L1 to_idx == 1 (exit), an index outside the state, amount_f or load_amount_f >= 2^40, from_eth_addr
 *                       >= 2^160, an L1 amount != 0 with to_idx == 0 (no receiver to update), n_l1 > HZ_LEDGER_MAX_L1, too many updates
 *                       (the L1 events count towards the 65536).
 *   hz_ledger_plan_batch  DIAGNOSTIC, no device: hz_ledger_plan_l2's outputs over the n_l1 + m rows (events of an L1 row: sender, then
 *                       receiver when amount != 0; fee_slot -1), plus the dense local slots of the accounts the L1 run touches, numbered
 *                       by first appearance: l1_slot_sender_out / l1_slot_receiver_out [n_l1] (-1: no receiver), *n_slots_out,
 *                       slot_account_out (room for 2 n_l1). Every output may be NULL
 *   hz_ledger_l1_flags_dev  the flag bytes as a DEVICE pointer, [n_l1] of the last successful hz_ledger_apply_batch, valid until the
 *                       ledger's next call
 *   hz_ledger_l1_ms     device time of the L1 kernel of the last hz_ledger_apply_batch (0: n_l1 was 0, the call did not succeed, or the
 *                       ledger has been used otherwise since)
 * EXITS. A row with to_idx == 1 is an exit: an L2 exit, or an L1 forceExit. The five apply calls above keep refusing it
 * with HZ_ERR_ARG; hz_ledger_apply_batch_exits accepts it. The sender side of an exit is exactly that of a transfer (L2: reasons 1, 2, 3
 * and 12, the fee to its slot, nonce + 1; L1: the nullifiers above, no fee, no nonce), and the state root after the row is the root after
 * the sender's update. Processor 2 works on the batch's EXIT TREE, an hz_smt the ledger owns, empty at the start of every batch, at key
 * from_idx:
 *   amount == 0 (the float40's mantissa is zero): a NOP, no exit-tree operation; the leaf-2 rows are as in a transfer (tokenID2 = token_id
 *                       for L2, all zero for L1), newExit = 0
 *   amount != 0, key not yet in the exit tree: INSERT, newExit = 1. The new leaf is {tokenID, sign, ay, ethAddr} of the SENDER's leaf, nonce
 *                       0, balance eff3 -- the amount for L2, eff3 above for L1 (0 when the amount is nullified; the insert still
 *                       happens). All six leaf-2 rows are zero; isOld0_2, oldKey2, oldValue2 are the tree's, as hz_smt_apply reports them
 *                       (oldKey2 = oldValue2 = 0 where isOld0_2 = 1)
 *   amount != 0, key present: UPDATE, newExit = 0. The leaf-2 rows are the exit leaf before; balance += eff3; isOld0_2 = oldKey2 = oldValue2 = 0
 * The receiver's token of an exit is the sender's: null_amount = null_eth || (null_tok1 && amount != 0) for a forceExit, and reason 4 cannot
 * fire on an L2 exit. Reason 5 holds for the exit leaf too: a new exit balance >= 2^192 refuses the batch at that row. siblings2 of an
 * exit row are the exit tree's, zero-padded to n_sib. txCompressedData, txCompressedDataV2 and the signed message carry to_idx = 1.
 *   hz_ledger_apply_batch_exits  hz_ledger_apply_batch with to_idx == 1 accepted in L1 and L2 rows, plus exit_out (may be NULL; nullable host
 *                       pointers): new_exit, is_old0_2, old_key2, old_value2 and exit_root_after as [n_l1 + m] 32-byte elements,
 *                       new_exit_root [1]. exit_root_after is the exit root after every row -- 0 until the first insert, unchanged
 *                       across rows without an exit operation; its first rows - 1 entries are imExitRoot. With no exit row every
 *                       output of hz_ledger_apply_batch is equal byte for byte and the exit arrays are zero. Exit operations count
 *                       towards the 65536 updates. HZ_ERR_ARG beyond hz_ledger_apply_batch's: an exit leaf that would lie at depth
 *                       >= n_sib (found by the planner, before anything is launched)
 *   hz_ledger_exit_outputs_dev  exit_out's arrays as DEVICE pointers of the last successful hz_ledger_apply_batch_exits, valid until the
 *                       ledger's next call; fit for hz_set_input_dev
 *   hz_ledger_exit_tree the exit tree, borrowed: hz_smt_proofs / _root / _size work on it (hz_smt_apply / _reset on it would leave the
 *                       exit leaves behind: do not)
 *   hz_ledger_exit_accounts  the fields (e0, balance, ay, ethAddr) of n exit leaves by key: fields_out [n][4][32]; a key that is not in
 *                       the exit tree is HZ_ERR_ARG
 *   hz_ledger_plan_exits  DIAGNOSTIC, no device: the plan of such a batch. An exit row makes its sender event and NO receiver event
 *                       (ev_receiver -1; last_event counts state events only); the exit operations are a second ordered list: per row
 *                       ev_exit_out (operation or -1) and last_exit_out (the last operation of rows 0 .. i, -1 none yet), per operation
 *                       (room for n_l1 + m) exit_row_out, exit_key_out, exit_prev_out (the previous operation on the same key, -1: the
 *                       operation is the insert), exit_perm_out (the operations grouped by key, groups by first appearance), and the
 *                       exit tree's own plan: exit_insert_out, exit_is_old0_out, exit_old_key_out. Every output may be NULL
 *   hz_ledger_exit_ms   device time of the exit kernels plus the exit tree's update of the last hz_ledger_apply_batch_exits (0: no exit
 *                       operation, or the call did not succeed). The update runs on the exit tree's own stream beside the state
 *                       tree's: the time is not a part of hz_ledger_device_ms that could be subtracted
 * LIFETIME. The exit tree and the exit leaves are those of the last successful call that applied a batch: every apply call (all six)
 * starts by emptying them, so after a refused call, and after a call of the other five, the tree is empty. A refused call leaves root,
 * planes and state tree untouched, as above.
 * EXIT TREES KEPT. A withdrawal is made against the exit tree of an EARLIER batch: the contract keeps one exit root per batch
 * number. hz_ledger_exit_keep freezes the exit tree as it stands under a batch number before the next apply call empties it; the frozen
 * trees -- the ARCHIVE -- lie in device memory the ledger owns, and the inputs of Withdraw(nLevels) come out of them in bulk:
 *   hz_ledger_exit_keep the exit tree and the exit leaves as they stand, kept under batch_num: after a successful
 *                       hz_ledger_apply_batch_exits / _creates / _atomic the batch's, after any other apply call or a refused one the
 *                       empty tree (a legitimate entry: exit root 0, no leaf). batch_num must be above every kept number (HZ_ERR_ARG). The
 *                       live exit tree, root, planes and the *_dev outputs of earlier calls stay as they are. A device allocation that
 *                       fails is HZ_ERR_HIP and the keep did not happen: the archive is unchanged. A ledger that never calls this
 *                       allocates nothing for the archive
 *   hz_ledger_exit_forget  drops every kept batch with a number below below_batch; its memory is free for later keeps once every
 *                       batch that shares its slab of device memory is forgotten too
 *   hz_ledger_exit_kept the kept batch numbers, ascending: the first cap of them into batch_out, *n the number kept
 *   hz_ledger_exit_archive_stats  kept snapshots, device slabs, the bytes the snapshots fill and the bytes reserved (slabs plus the
 *                       descriptor table). Every output may be NULL
 *   hz_ledger_exit_root_of  the exit root of a kept batch (HZ_ERR_ARG: not kept)
 *   hz_ledger_withdraw_rows  n <= 2^20 queries (batch_num[i], idx[i]) in any order, over any mix of kept batches, for Withdraw(n_levels):
 *                       out (may be NULL; nullable host pointers) takes the circuit's input signals row-major, as hz_set_input(...,
 *                       instance = -1, ...) wants them for a context of n instances: root_exit, eth_addr, token_id, balance, idx, sign, ay
 *                       [n][32], siblings_state [n][n_levels + 1][32] zero-padded, and status [n] bytes:
 *                         0 found        1 batch_num is not kept        2 idx is not in that tree (the walk met nothing or another leaf,
 *                         or idx >= 2^48)        3 the leaf needs n_levels + 1 or more siblings (hz_smt_proofs' depth rule)
 *                       Every row of a query whose status is not 0 is zero. tokenID and sign are unpacked from the leaf's e0 on the
 *                       device. Like hz_ledger_verify_l2 the call refuses nothing but arguments -- HZ_ERR_ARG: a null argument, n above
 *                       2^20, n_levels + 1 outside 1 .. 64 -- changes nothing resident and invalidates the *_dev outputs of earlier calls
 *   hz_ledger_withdraw_rows_dev  the same nine arrays as DEVICE pointers of the last hz_ledger_withdraw_rows, valid until the ledger's
 *                       next call; fit for hz_set_input_dev
 *   hz_ledger_withdraw_ms / hz_ledger_exit_keep_ms  device time of the two kernels of the last hz_ledger_withdraw_rows; of the copies of
 *                       the last hz_ledger_exit_keep
 * The archive lives as long as the loaded state: hz_ledger_load / hz_ledger_load_accounts empty it. It works on dense and growing ledgers.
 * CREATES. An L1 row with from_idx == 0 creates an account: createAccount, createAccountDeposit,
 * createAccountDepositTransfer, and the coordinator's L1 transactions. The state tree's shape changes, so only a GROWING ledger takes one:
 *   hz_ledger_create_growing  a ledger of up to `capacity` accounts (1 .. 2^24; first_idx >= 2) whose state tree is an hz_smt of n_sib_max siblings it
 *                       owns. The four planes are allocated once, [capacity][32] each; they do not grow by reallocation. hz_ledger_tree
 *                       is NULL for it, hz_ledger_state_smt the tree. n_sib of every call: 1 .. n_sib_max; there is no k <= n_sib
 *                       rule -- a leaf that would lie at depth >= n_sib is HZ_ERR_ARG from the tree's planner, before the update is launched
 *   hz_ledger_load_accounts  0 <= n <= capacity consecutive accounts first_idx .. first_idx + n - 1 (n == 0: the genesis state, root 0).
 *                       hz_ledger_load's leaf-range checks, first offender named, nothing touched; every field below r. A reload
 *                       resets the tree first. hz_ledger_load is for dense ledgers, this call for growing ones
 *   hz_ledger_size / _last_idx  live accounts; first_idx + size - 1 (first_idx - 1 when empty). Both kinds of ledger
 *   hz_ledger_state_smt the state tree, borrowed: hz_smt_proofs / _root / _size work on it; NULL on a dense ledger
 * All apply / verify / resolve calls above work on a growing ledger, over its live accounts, and keep refusing from_idx == 0; on the same
 * 2^k accounts every output equals the dense ledger's byte for byte. After a HIP failure reported behind the state tree's queued
 * write-back a growing ledger answers HZ_ERR_HIP until it is loaded again (hz_smt_apply's rule).
 *   hz_ledger_apply_batch_creates  hz_ledger_apply_batch_exits with from_idx == 0 accepted in L1 rows. from_bjj[n_l1][32]: fromBjjCompressed
 *                       of every L1 row, little-endian, read only where from_idx == 0 (NULL when no row creates). Row i creates account
 *                       auxFromIdx = last idx + 1, last idx running over the rows. The new leaf: tokenID = token_id, nonce 0, ethAddr =
 *                       from_eth_addr, sign = bit 255 of the key, ay = its bits 0 .. 253 reduced once modulo r (bit 254 is not read),
 *                       balance 0. No nullifier applies to the load or the sender side; then the L1 arithmetic above runs from balance 0:
 *                       eff_load = loadAmount, null_amount = amount != 0 && token_id != receiver's tokenID, underflow_ok, eff3,
 *                       isAmountNullified as above. Processor 1 is an INSERT of the leaf after the row; the leaf-1 rows are the new
 *                       leaf with balance 0, siblings1 those of the walk before the insert. Processor 2 is the L1 run's. A created
 *                       account exists for every later row and for its own row's to_idx (a self-transfer): later L1 rows, L2 senders
 *                       (signature verified against the new key), L2 receivers by index, address or key (the lowest index over live
 *                       plus created accounts wins), L2 exits, fee slots. create_out (may be NULL; nullable host pointers):
 *                       aux_from_idx, is_old0_1, old_key1, old_value1 [n_l1 + m] (zero for a row that creates nothing; old_key1 =
 *                       old_value1 = 0 where is_old0_1 = 1), out_idx_after [n_l1 + m] (its first rows - 1 entries are imOutIdx),
 *                       new_last_idx [1]. With no create row every output equals hz_ledger_apply_batch_exits' byte for byte, on either
 *                       kind of ledger. A refused call does not raise the size. HZ_ERR_ARG beyond hz_ledger_apply_batch_exits': a create
 *                       row on a dense ledger, from_bjj == NULL with a create row, size + creates > capacity, an L1 from_idx or to_idx
 *                       above the row's current last idx (a create row: above its own new idx), a create row with to_idx == 1 or
 *                       with an amount and to_idx == 0, a leaf at depth >= n_sib
 *   hz_ledger_create_outputs_dev  create_out's arrays as DEVICE pointers of the last successful hz_ledger_apply_batch_creates
 *   hz_ledger_create_ms device time of the two create kernels of the last hz_ledger_apply_batch_creates
 *   hz_ledger_plan_creates  DIAGNOSTIC, no device: aux_from_idx_out / out_idx_after_out [n_l1 + m], *n_creates_out, and the argument errors
 *                       above but the depth, for a ledger of `capacity` that holds `size` accounts (growing == 0: a dense one)
 * ATOMIC. An L2 transaction may commit to a partner: its signer puts the partner's txCompressedDataV2, signed toEthAddr and
 * signed toBjjAy -- the partner's LINK FIELDS -- into the message, M = Poseidon(6)(txCompressedData, e1, toBjjAy, rqTxCompressedDataV2,
 * rqToEthAddr, rqToBjjAy), and the coordinator names with rqOffset where in the batch the partner stands. RollupMain accepts the batch only
 * if the three rq fields of every row equal, as full field elements, the link fields of its target (src/rq-tx-verifier.circom:91-93):
 *   rq_offset 0: nothing, the comparison is against (0, 0, 0)    1 .. 3: row r + k    4 .. 7: row r - (8 - k) (7 the previous row, 4 four back)
 * over the batch's n_l1 + m rows, L1 first (L2 transaction i is row r = n_l1 + i). An L1 row, an L2 NOP and a position before row 0 or past
 * the last row have link fields (0, 0, 0): a link there, and offset 0, hold iff the three rq fields are zero. An rq_to_eth_addr >= 2^160 never
 * matches. The link fields of an active L2 row are those of its signed values: to_idx as signed (0 and 1 included) and to_bjj_sign in V2,
 * to_eth_addr and to_bjj_ay of its hz_l2sig. The rq fields are always explicit -- what the signer committed to -- and a NOP's hz_l2rq is
 * ignored. The seven apply / verify / resolve calls above know no link: their message keeps three zeros, and they know no reason 13.
 *   hz_ledger_apply_batch_atomic  hz_ledger_apply_batch_creates with rq[m] (entry i belongs to txs[i]; NULL: no transaction links; where
 *                       sigs may be NULL there it may be here, and the link fields of every row are then V2 and two zeros), on a
 *                       dense or a growing ledger. sig_l2_hash is the M above. Refusal reason
 *                         13 the rq fields of the row are not its target's link fields
 *                       ranks with 1 - 8 and 12 (lowest row, then lowest reason; reason 9 keeps its precedence) and is checked with or
 *                       without HZ_LEDGER_VERIFY_SIGS: the circuit enforces it whoever verified a signature. A signature over other rq
 *                       fields than the submitted ones is reason 7 under the flag. With rq == NULL, or every entry zero, every output
 *                       equals hz_ledger_apply_batch_creates' byte for byte. HZ_ERR_ARG beyond that call's: rq_offset > 7.
 *                       HZ_ERR_INPUT: an rq field >= r
 *   hz_ledger_verify_l2_atomic  hz_ledger_verify_l2 with rq[m]: the rows are the m transactions alone (n_l1 = 0). Verdicts 0, 7, 8 or 13, the
 *                       lowest where several hold. A rejection is not carried over to the partner of the rejected transaction
 *   hz_ledger_plan_atomic  DIAGNOSTIC, no device: target_row_out[m], the row a transaction is compared with, or -1 for zeros (offset 0, a
 *                       position outside the batch, an L1 row, a NOP); verdict_out[m], 0 or 13, computed on the host with the routines the
 *                       kernel uses; the argument errors above. Both outputs may be NULL
 *   hz_ledger_rq_ms     device time of the link kernel of the last such call (0: none ran)
 * SELECT. The calls above take a batch somebody has chosen; hz_ledger_select_batch chooses one from a POOL of m candidate L2
 * transactions in the caller's order of preference, over the resident state and behind the same mandatory L1 rows: it keeps what is
 * applicable after everything kept before it and DROPS the rest with a reason, where the calls above refuse. L1 rows run first and are
 * nullified as in 8f, never dropped. partner[i] (or NULL: none) is the POOL index of the transaction that transaction i requires, -1 for
 * none; rq[i].rq_offset is ignored (positions do not survive a drop), the three rq fields stay what the signer committed to.
 *   STATIC verdicts, from the planes as they are before the batch plus the slots of created accounts: 1 the sender's token differs; 4 the
 *   receiver's token differs and the amount is not zero; 7 / 8 from the signature kernels under HZ_LEDGER_VERIFY_SIGS; 9 to_idx == 0 with an
 *   amount and no account among live plus created holds the signed destination; 13 partner[i] >= 0 and the rq fields are not that
 *   transaction's link fields, or partner[i] < 0 and an rq field is not zero; 16 the fee is 2^128 or more (amount and selector alone).
 *   THE WALK goes in pool order over the balances and nonces the L1 run left. A transaction is kept when it has no static verdict, is not
 *   forced out, fewer than max_keep are kept so far, its nonce is the sender's current nonce (else 2), that nonce is not 2^40 - 1 (else
 *   12), balance >= amount + fee (else 3) and the receiver's new balance stays below 2^192 (else 5). A kept transaction debits its sender
 *   by amount + fee -- whether or not a fee slot would take the fee -- raises its nonce, and credits the receiver when the amount is not
 *   zero and the row is not an exit (a self-transfer sees the sender's new balance). A dropped transaction leaves no trace.
 *   THE VERDICT byte: 0 kept; else the reason hz_ledger_apply_batch_atomic names when that transaction is the one it refuses -- 9 where 9
 *   holds, otherwise the lowest reason that holds, static or not, on the state the walk has reached; HZ_SELECT_PARTNER (14) forced out by
 *   the closure below (it ranks before a reason: the transaction was valid when a walk reached it); HZ_SELECT_FULL (15) nothing holds
 *   but max_keep are kept. A pool NOP (from_idx == 0) gets 0, is not kept and not counted; its partner entry is not read.
 *   CLOSURE over links. After a walk a kept transaction is forced out when its partner is not kept, or when the partner's distance d in
 *   the compacted batch (row of the partner minus its own, kept transactions only) is no offset: d = 1 .. 3 is offset d, d = -4 .. -1
 *   offset 8 + d. If anything was forced out the walk runs again from the L1 run's balances with the forced set added; the set only
 *   grows, so there are at most (linked transactions + 1) walks, and *rounds is their number. The result is defined by this procedure
 *   and nothing else. Links are one-directional: a dropped requirer does not drop a partner that does not require it.
 *   hz_ledger_select_batch  out's members are nullable host pointers: verdict[m]; kept[m], pool indices in order, *n_kept of them valid;
 *                       rq_offset[m], for a kept transaction its offset in the compacted batch (0 without a partner); aux_to_idx[m], the
 *                       receiver the lookup found (0: none asked for or none found); *rounds. sigs may be NULL where
 *                       hz_ledger_apply_batch_atomic allows it. HZ_ERR_ARG beyond that call's: partner[i] == i or outside -1 .. m - 1; m >
 *                       HZ_SELECT_MAX_POOL or more than HZ_SELECT_MAX_SLOTS distinct accounts among the L1 rows and the pool, naming the
 *                       first pool index that does not fit. HZ_ERR_INPUT: an L1 row that refuses the batch (reason 5), named as apply does
 *                       CONTRACT. The call changes nothing resident: root, planes below size, size. It may write plane slots beyond size,
 *                       as a refused hz_ledger_apply_batch_creates does. It does not touch the exit tree. It invalidates the *_dev
 *                       outputs of earlier calls, as hz_ledger_verify_l2 does. A later hz_ledger_apply_batch_atomic over the same L1
 *                       rows and the kept transactions, compacted and carrying rq_offset, with the same flags, is not refused for
 *                       reasons 1 - 5, 7 - 9, 12, 13 or 16 at an L2 row. Still possible, and not this call's business: reason 6 and reason
 *                       5 at a fee slot (both depend on a fee plan the call never sees) and the tree planners' depth errors
 *   hz_ledger_plan_select  DIAGNOSTIC, no device: the local slot of every L1 row's and pool transaction's sender and receiver (-1: none;
 *                       aux_to_idx[m] or NULL stands for the lookup: a to_idx == 0 row takes its receiver from there, 0 or NULL: none),
 *                       the accounts of the slots, the argument errors above (the state is not known here: an L1 row that creates an
 *                       account is given with its auxFromIdx in from_idx's place, from_idx == 0 is HZ_ERR_ARG); and, given kept_in[m], the closure step alone --
 *                       forced_out[m] and rq_offset_out[m] -- by the routine the kernel runs. Every output may be NULL
 *   hz_ledger_select_ms device time of k_ledger_select in the last hz_ledger_select_batch
 * MAIN INPUTS. After a successful apply call that carried a chain id -- every one but hz_ledger_apply_l2 -- and before the
 * ledger's next call, hz_ledger_main_inputs writes the PACKED input buffer (hz_inputs_packed_bytes, above) of one instance of a
 * RollupMain(nTx, nLevels, maxL1Tx, maxFeeTx) context on the ledger's device into device memory of the caller: every input signal, in
 * hz_input_name order and at hz_input_packed_offset, byte for byte what the host route builds from the same request and the apply's
 * host outputs. The state-dependent signals are copied from where the apply left them (imStateRoot / imAccFeeOut / imExitRoot / imOutIdx
 * the first nTx - 1 rows of their arrays, imInitStateRootFee row nTx - 1 of state_root_after, imStateRootFee the first maxFeeTx - 1 rows;
 * zeros for the exit signals of a call without exits, zeros and old_last_idx in every imOutIdx row for a call without creates); oldLastIdx
 * is old_last_idx, oldStateRoot, globalChainID, currentNumBatch, feeIdxs and feePlanTokens are the call's; the transaction-only signals
 * are packed from the uploaded rows: an L1 row has onChain 1, the caller's fromIdx (0 and newAccount 1 on a create row), toIdx,
 * amountF, loadAmountF, fromEthAddr, txCompressedData = the signature constant | chain id << 32 | fromIdx << 48 | toIdx << 96 | tokenID
 * << 144, and the 256 bits of from_bjj[i] in fromBjjCompressed (zeros for from_bjj == NULL); an L2 row has txCompressedData and
 * txCompressedDataV2 as the signature kernels pack them, the caller's amountF, fromIdx and toIdx, toBjjAy, toEthAddr, maxNumBatch, s, r8x
 * and r8y of its hz_l2sig entry (zeros for sigs == NULL), rqOffset and the three rq fields of its hz_l2rq entry (zeros for rq == NULL); a NOP row is
 * zero but for the constant and the chain id; imOnChain is onChain without its last row.
 *   hz_ledger_main_inputs  bytes == hz_inputs_packed_bytes(ctx); d_packed is device memory, 32-byte aligned. Every byte of [0, bytes) is
 *                       written. HZ_ERR_ARG: a null argument; no successful apply call with a chain id since the ledger's last other
 *                       call (none yet, a refused one, hz_ledger_apply_l2, or a call that invalidates the *_dev outputs); ctx is no
 *                       rollup-main context or lies on another device; n_l1 + m != nTx, n_l1 > maxL1Tx, F != maxFeeTx, n_sib !=
 *                       nLevels + 1; bytes is not the packed size; on a growing ledger, old_last_idx is not the ledger's last idx
 *                       before the batch. The target buffer is untouched then.
 *                       CONTRACT. The call changes nothing resident, invalidates no *_dev output and refuses nothing but arguments. It
 *                       returns once its kernel has finished (one synchronise on the ledger's stream): d_packed may then go to
 *                       hz_inputs_stage / _stage_range / _upload on any stream, and an element >= r in it is reported by the next
 *                       hz_witness_check. It may be called again for another buffer
 *   hz_ledger_main_inputs_ms  device time of its kernel in the last such call
 *   hz_ledger_plan_main_inputs  DIAGNOSTIC, no device: the descriptor table of a layout given as plain arrays (names, offsets, widths,
 *                       flat lengths; bytes its size), a shape and the call's HZ_MI_* flags, by the routine the device call uses: per
 *                       signal kind_out (HZ_MI_KIND_*), source_out (HZ_MI_SRC_*), first_row_out and rows_out. HZ_ERR_ARG: an unknown
 *                       or repeated signal name, a missing one, a width or flat length that does not fit the shape, a range that is
 *                       not 32-byte aligned, overlaps another or ends beyond bytes
 * ROLLBACK. `applied` -- a MARK -- is the number of successful apply calls since the ledger's last load: all seven forms
 * count, hz_ledger_apply_l2 included; a refused call, hz_ledger_verify_*, _resolve_l2, _select_batch, _withdraw_rows, _main_inputs and
 * _exit_keep do not; a load sets it to 0 and empties the journal. It counts whether or not a journal is on.
 *   hz_ledger_journal   keeps an undo record of each of the last `depth` applies (0 .. HZ_LEDGER_JOURNAL_MAX; 0, the default of a new
 *                       ledger, turns the journal off and frees its memory). Every call discards the records held. With the journal off
 *                       an apply launches no kernel and allocates nothing for it. With it on, an apply saves the resident 32-byte elements its
 *                       write-backs replace -- touched tree nodes and state hashes (pool entries of a growing ledger), the four plane
 *                       elements of every touched account -- into a ring of depth + 1 device slabs of one capacity, grown by doubling
 *                       when a record does not fit: an apply allocates only then
 *   hz_ledger_applied   *mark = applied. HZ_ERR_ARG: a null argument
 *   hz_ledger_rollback  makes the ledger what it was when hz_ledger_applied gave `mark`, byte for byte: the root, every plane element
 *                       below the size, the size of a growing ledger, every resident entry of the state tree (levels and state hashes;
 *                       shape and the node, leaf and value pools). The records are undone newest first on the ledger's stream, one
 *                       synchronise at the end. Afterwards the batch's exit tree is empty, as after a load; every exit tree kept after
 *                       `mark` was reached is dropped (a record notes the highest kept batch_num when its apply began: snapshots above it
 *                       go, their bytes released as hz_ledger_exit_forget releases them; those kept before stay and answer
 *                       hz_ledger_withdraw_rows as before); every *_dev output and the hz_ledger_main_inputs window are invalid;
 *                       applied == mark and the records above mark are gone. mark == applied succeeds and changes and invalidates
 *                       nothing. HZ_ERR_ARG, nothing changed: a null ledger, a ledger not loaded, mark > applied, mark < applied - records
 *                       (the journal is off, or the ring has moved on); the message names both numbers. A HIP failure after the first
 *                       restore was queued leaves the ledger answering HZ_ERR_HIP until it is loaded again
 *   hz_ledger_journal_stats  the depth, the records held, the oldest mark hz_ledger_rollback accepts, the bytes the records fill and the
 *                       bytes the slabs reserve; every output may be NULL
 *   hz_ledger_journal_ms / _rollback_ms  device time of the save kernels in the last apply (0 with the journal off) / of the last rollback
 * OUT OF SCOPE: L1 transactions that create accounts or exit through a call other than hz_ledger_apply_batch_exits (creates:
 * hz_ledger_apply_batch_creates on a growing ledger), an L1 amount with
 * to_idx == 0 (no receiver), persisting, or carrying across a reload, the exit trees of earlier batches kept resident, a resident address index kept across
 * calls, batch (random linear combination) verification of signatures, more than one device per ledger, the packed inputs of
 * hz_ledger_apply_l2 (it has no chain id) or of more than one batch per hz_ledger_main_inputs call (K applies go into K consecutive
 * slots of one buffer, staged with hz_inputs_stage_range), writing straight into the witness layout; restoring the live exit tree of the batch rolled back to
 * (keep it first), undo records that outlive the process or a reload. One thread at a time. */
typedef struct hz_ledger hz_ledger;
typedef struct {
    uint64_t from_idx, to_idx, amount_f /* float40 */, nonce;
    uint32_t token_id;
    uint8_t user_fee;
} hz_l2tx;
#define HZ_LEDGER_ARRAYS 27
typedef struct {
    uint8_t *tokenID1, *nonce1, *sign1, *balance1, *ay1, *ethAddr1; /* [m]: the sender BEFORE; zero for a NOP */
    uint8_t* siblings1;                                             /* [m][n_sib] */
    uint8_t *tokenID2, *nonce2, *sign2, *balance2, *ay2, *ethAddr2; /* [m]: the receiver before processor 2 */
    uint8_t* siblings2;                                             /* [m][n_sib] */
    uint8_t* state_root_after;                                      /* [m]: unchanged across a NOP; its first m - 1 rows are imStateRoot */
    uint8_t* acc_fee_after;                                         /* [m][F]: imAccFeeOut */
    uint8_t *tokenID3, *nonce3, *sign3, *balance3, *ay3, *ethAddr3; /* [F]: the fee receiver before its update; zero for an unused slot */
    uint8_t* siblings3;                                             /* [F][n_sib] */
    uint8_t* state_root_after_fee;                                  /* [F]: imStateRootFee is its first F - 1 rows */
    uint8_t* final_acc_fee;                                         /* [F]: imFinalAccFee */
    uint8_t *old_root, *new_root;                                   /* [1] each; imInitStateRootFee is state_root_after[m - 1] */
} hz_ledger_out;
hz_status hz_ledger_create(int32_t device, int32_t k, uint64_t first_idx, hz_ledger** out);
void hz_ledger_destroy(hz_ledger* l);
hz_status hz_ledger_load(hz_ledger* l, const uint8_t* e0, const uint8_t* balance, const uint8_t* ay, const uint8_t* eth_addr);
hz_status hz_ledger_root(hz_ledger* l, uint8_t* out32);
hz_status hz_ledger_accounts(hz_ledger* l, size_t n, const uint64_t* idx, uint8_t* fields_out);
hz_state* hz_ledger_tree(hz_ledger* l);
hz_status hz_ledger_apply_l2(hz_ledger* l, size_t m, const hz_l2tx* txs, size_t F, const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs,
                             size_t n_sib, const hz_ledger_out* out);
hz_status hz_ledger_outputs_dev(hz_ledger* l, hz_ledger_out* dev);
hz_status hz_ledger_plan_l2(size_t m, const hz_l2tx* txs, size_t F, const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs, int32_t k,
                            uint64_t first_idx, int32_t* ev_sender_out, int32_t* ev_receiver_out, int32_t* fee_slot_out, int32_t* last_event_out,
                            size_t* n_events_out, uint64_t* ev_account_out, int32_t* ev_prev_out);
double hz_ledger_device_ms(const hz_ledger* l);
double hz_ledger_semantic_ms(const hz_ledger* l);
typedef struct {
    uint8_t s[32], r8x[32], r8y[32]; /* canonical little-endian */
    uint8_t to_eth_addr[32], to_bjj_ay[32];
    uint32_t max_num_batch;
    uint8_t to_bjj_sign;
} hz_l2sig;
typedef struct {
    uint8_t *tx_compressed_data, *tx_compressed_data_v2, *sig_l2_hash; /* [m] each, nullable */
} hz_ledger_sig_out;
hz_status hz_ledger_apply_l2_signed(hz_ledger* l, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, uint32_t chain_id, uint32_t current_num_batch,
                                    size_t F, const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs, size_t n_sib, const hz_ledger_out* out,
                                    const hz_ledger_sig_out* sig_out);
hz_status hz_ledger_verify_l2(hz_ledger* l, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, uint32_t chain_id, uint32_t current_num_batch,
                              uint8_t* verdict_out /* [m]: 0, 7 or 8 */, const hz_ledger_sig_out* sig_out);
hz_status hz_ledger_sig_outputs_dev(hz_ledger* l, hz_ledger_sig_out* dev);
double hz_ledger_sig_ms(const hz_ledger* l);
#define HZ_LEDGER_VERIFY_SIGS 1u
hz_status hz_ledger_apply_l2_addr(hz_ledger* l, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, uint32_t flags,
                                  const uint64_t* aux_to_idx /* [m] or NULL */, uint32_t chain_id, uint32_t current_num_batch, size_t F,
                                  const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs, size_t n_sib, const hz_ledger_out* out,
                                  const hz_ledger_sig_out* sig_out, uint8_t* aux_to_idx_out /* [m][32] or NULL */);
hz_status hz_ledger_resolve_l2(hz_ledger* l, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, uint64_t* aux_to_idx_out /* [m] */);
hz_status hz_ledger_aux_to_idx_dev(hz_ledger* l, uint8_t** dev);
double hz_ledger_resolve_ms(const hz_ledger* l);
typedef struct {
    uint64_t from_idx, to_idx, amount_f /* float40 */, load_amount_f /* float40 */;
    uint32_t token_id;
    uint8_t from_eth_addr[32]; /* little-endian, below 2^160 */
} hz_l1tx;
#define HZ_LEDGER_MAX_L1 512
hz_status hz_ledger_apply_batch(hz_ledger* l, size_t n_l1, const hz_l1tx* l1, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, uint32_t flags,
                                const uint64_t* aux_to_idx /* [m] or NULL */, uint32_t chain_id, uint32_t current_num_batch, size_t F,
                                const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs, size_t n_sib, const hz_ledger_out* out /* n_l1 + m rows */,
                                const hz_ledger_sig_out* sig_out /* [m], L2 rows */, uint8_t* aux_to_idx_out /* [n_l1 + m][32] or NULL */,
                                uint8_t* l1_flags_out /* [n_l1] or NULL: bit 0 nullifyLoadAmount, bit 1 isAmountNullified */);
hz_status hz_ledger_plan_batch(size_t n_l1, const hz_l1tx* l1, size_t m, const hz_l2tx* txs, size_t F, const uint32_t* fee_plan_tokens,
                               const uint64_t* fee_idxs, int32_t k, uint64_t first_idx, int32_t* ev_sender_out, int32_t* ev_receiver_out,
                               int32_t* fee_slot_out, int32_t* last_event_out, size_t* n_events_out, uint64_t* ev_account_out, int32_t* ev_prev_out,
                               int32_t* l1_slot_sender_out, int32_t* l1_slot_receiver_out, size_t* n_slots_out, uint64_t* slot_account_out);
hz_status hz_ledger_l1_flags_dev(hz_ledger* l, uint8_t** dev);
double hz_ledger_l1_ms(const hz_ledger* l);
#define HZ_LEDGER_EXIT_ARRAYS 6
typedef struct {
    uint8_t *new_exit, *is_old0_2, *old_key2, *old_value2; /* [n_l1 + m]: zero for a row without an exit operation */
    uint8_t* exit_root_after;                              /* [n_l1 + m]: its first n_l1 + m - 1 rows are imExitRoot */
    uint8_t* new_exit_root;                                /* [1] */
} hz_ledger_exit_out;
hz_status hz_ledger_apply_batch_exits(hz_ledger* l, size_t n_l1, const hz_l1tx* l1, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, uint32_t flags,
                                      const uint64_t* aux_to_idx /* [m] or NULL */, uint32_t chain_id, uint32_t current_num_batch, size_t F,
                                      const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs, size_t n_sib, const hz_ledger_out* out,
                                      const hz_ledger_sig_out* sig_out, uint8_t* aux_to_idx_out, uint8_t* l1_flags_out,
                                      const hz_ledger_exit_out* exit_out /* or NULL */);
hz_status hz_ledger_exit_outputs_dev(hz_ledger* l, hz_ledger_exit_out* dev);
hz_smt* hz_ledger_exit_tree(hz_ledger* l);
hz_status hz_ledger_exit_accounts(hz_ledger* l, size_t n, const uint64_t* key, uint8_t* fields_out /* [n][4][32] */);
hz_status hz_ledger_plan_exits(size_t n_l1, const hz_l1tx* l1, size_t m, const hz_l2tx* txs, size_t F, const uint32_t* fee_plan_tokens,
                               const uint64_t* fee_idxs, int32_t k, uint64_t first_idx, size_t n_sib, int32_t* ev_sender_out, int32_t* ev_receiver_out,
                               int32_t* last_event_out, size_t* n_events_out, uint64_t* ev_account_out, int32_t* ev_exit_out, int32_t* last_exit_out,
                               size_t* n_exits_out, uint32_t* exit_row_out, uint64_t* exit_key_out, int32_t* exit_prev_out, uint32_t* exit_perm_out,
                               uint8_t* exit_insert_out, uint8_t* exit_is_old0_out, uint64_t* exit_old_key_out);
double hz_ledger_exit_ms(const hz_ledger* l);
#define HZ_WITHDRAW_ARRAYS 9
#define HZ_WITHDRAW_MAX_ROWS ((size_t)1 << 20)
typedef struct {
    uint8_t *root_exit, *eth_addr, *token_id, *balance, *idx, *sign, *ay; /* [n]: Withdraw's inputs (src/withdraw.circom:26-33) */
    uint8_t* siblings_state;                                              /* [n][n_levels + 1] */
    uint8_t* status;                                                      /* [n] BYTES: 0 found, 1 not kept, 2 absent, 3 too deep */
} hz_withdraw_rows_out;
hz_status hz_ledger_exit_keep(hz_ledger* l, uint32_t batch_num);
hz_status hz_ledger_exit_forget(hz_ledger* l, uint32_t below_batch);
hz_status hz_ledger_exit_kept(const hz_ledger* l, uint32_t* batch_out /* [cap] */, size_t cap, size_t* n);
hz_status hz_ledger_exit_archive_stats(const hz_ledger* l, size_t* snapshots, size_t* slabs, size_t* bytes_used, size_t* bytes_reserved);
hz_status hz_ledger_exit_root_of(hz_ledger* l, uint32_t batch_num, uint8_t* out32);
hz_status hz_ledger_withdraw_rows(hz_ledger* l, size_t n, const uint32_t* batch_num, const uint64_t* idx, int32_t n_levels,
                                  const hz_withdraw_rows_out* out /* or NULL */);
hz_status hz_ledger_withdraw_rows_dev(hz_ledger* l, hz_withdraw_rows_out* dev);
double hz_ledger_withdraw_ms(const hz_ledger* l);
double hz_ledger_exit_keep_ms(const hz_ledger* l);
hz_status hz_ledger_create_growing(int32_t device, uint64_t capacity, uint64_t first_idx, int32_t n_sib_max, hz_ledger** out);
hz_status hz_ledger_load_accounts(hz_ledger* l, uint64_t n, const uint8_t* e0, const uint8_t* balance, const uint8_t* ay, const uint8_t* eth_addr);
uint64_t hz_ledger_size(const hz_ledger* l);
uint64_t hz_ledger_last_idx(const hz_ledger* l);
hz_smt* hz_ledger_state_smt(hz_ledger* l);
#define HZ_LEDGER_CREATE_ARRAYS 6
typedef struct {
    uint8_t *aux_from_idx, *is_old0_1, *old_key1, *old_value1; /* [n_l1 + m]: zero for a row that creates nothing */
    uint8_t* out_idx_after;                                    /* [n_l1 + m]: its first n_l1 + m - 1 rows are imOutIdx */
    uint8_t* new_last_idx;                                     /* [1] */
} hz_ledger_create_out;
hz_status hz_ledger_apply_batch_creates(hz_ledger* l, size_t n_l1, const hz_l1tx* l1, const uint8_t* from_bjj /* [n_l1][32] or NULL */, size_t m,
                                        const hz_l2tx* txs, const hz_l2sig* sigs, uint32_t flags, const uint64_t* aux_to_idx /* [m] or NULL */,
                                        uint32_t chain_id, uint32_t current_num_batch, size_t F, const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs,
                                        size_t n_sib, const hz_ledger_out* out, const hz_ledger_sig_out* sig_out, uint8_t* aux_to_idx_out,
                                        uint8_t* l1_flags_out, const hz_ledger_exit_out* exit_out /* or NULL */,
                                        const hz_ledger_create_out* create_out /* or NULL */);
hz_status hz_ledger_create_outputs_dev(hz_ledger* l, hz_ledger_create_out* dev);
double hz_ledger_create_ms(const hz_ledger* l);
hz_status hz_ledger_plan_creates(size_t n_l1, const hz_l1tx* l1, const uint8_t* from_bjj, size_t m, const hz_l2tx* txs, size_t F,
                                 const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs, int32_t growing, uint64_t capacity, uint64_t first_idx,
                                 uint64_t size, uint64_t* aux_from_idx_out, uint64_t* out_idx_after_out, size_t* n_creates_out);
typedef struct {
    uint8_t rq_tx_compressed_data_v2[32], rq_to_eth_addr[32], rq_to_bjj_ay[32]; /* canonical little-endian */
    uint8_t rq_offset;                                                           /* 0 .. 7 */
} hz_l2rq;
hz_status hz_ledger_apply_batch_atomic(hz_ledger* l, size_t n_l1, const hz_l1tx* l1, const uint8_t* from_bjj /* [n_l1][32] or NULL */, size_t m,
                                       const hz_l2tx* txs, const hz_l2sig* sigs, const hz_l2rq* rq /* [m] or NULL */, uint32_t flags,
                                       const uint64_t* aux_to_idx /* [m] or NULL */, uint32_t chain_id, uint32_t current_num_batch, size_t F,
                                       const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs, size_t n_sib, const hz_ledger_out* out,
                                       const hz_ledger_sig_out* sig_out, uint8_t* aux_to_idx_out, uint8_t* l1_flags_out,
                                       const hz_ledger_exit_out* exit_out /* or NULL */, const hz_ledger_create_out* create_out /* or NULL */);
hz_status hz_ledger_verify_l2_atomic(hz_ledger* l, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, const hz_l2rq* rq /* [m] or NULL */, uint32_t chain_id,
                                     uint32_t current_num_batch, uint8_t* verdict_out /* [m]: 0, 7, 8 or 13 */, const hz_ledger_sig_out* sig_out);
hz_status hz_ledger_plan_atomic(size_t n_l1, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, const hz_l2rq* rq /* [m] or NULL */,
                                int64_t* target_row_out /* [m]: the row, -1: zeros */, uint8_t* verdict_out /* [m]: 0 or 13 */);
double hz_ledger_rq_ms(const hz_ledger* l);
#define HZ_SELECT_MAX_POOL 4096  /* candidates in one hz_ledger_select_batch */
#define HZ_SELECT_MAX_SLOTS 4096 /* distinct accounts its L1 rows and pool may touch */
#define HZ_SELECT_PARTNER 14     /* verdicts of hz_ledger_select_batch that are no refusal reasons */
#define HZ_SELECT_FULL 15
#define HZ_LEDGER_FEE_OVERFLOW 16 /* refusal reason: amount x fee factor does not fit 128 bits (src/compute-fee.circom:89-91) */
typedef struct {
    uint8_t* verdict;     /* [m] */
    uint32_t* kept;       /* [m], *n_kept valid */
    size_t* n_kept;
    uint8_t* rq_offset;   /* [m] */
    uint64_t* aux_to_idx; /* [m] */
    uint32_t* rounds;
} hz_ledger_select_out;
hz_status hz_ledger_select_batch(hz_ledger* l, size_t n_l1, const hz_l1tx* l1, const uint8_t* from_bjj /* [n_l1][32] or NULL */, size_t m,
                                 const hz_l2tx* txs, const hz_l2sig* sigs, const hz_l2rq* rq /* [m] or NULL */, const int32_t* partner /* [m] or NULL */,
                                 uint32_t flags, uint32_t chain_id, uint32_t current_num_batch, size_t max_keep, const hz_ledger_select_out* out);
hz_status hz_ledger_plan_select(size_t n_l1, const hz_l1tx* l1, size_t m, const hz_l2tx* txs, const uint64_t* aux_to_idx /* [m] or NULL */,
                                const int32_t* partner /* [m] or NULL */, const uint8_t* kept_in /* [m] or NULL */, int32_t* slot_sender_out /* [n_l1 + m] */,
                                int32_t* slot_receiver_out /* [n_l1 + m] */, size_t* n_slots_out, uint64_t* slot_account_out /* [n_slots] */,
                                uint8_t* forced_out /* [m] */, uint8_t* rq_offset_out /* [m] */);
double hz_ledger_select_ms(const hz_ledger* l);
/* the kind flags of the call hz_ledger_plan_main_inputs plans for: hz_l2sig entries were given; hz_l2rq entries were given; the call
 * takes exits; it takes creates; it leaves auxToIdx rows (every call with a chain id but hz_ledger_apply_l2_signed); the ledger grows
 * (the table does not depend on it: the device call checks old_last_idx there) */
#define HZ_MI_SIGS 1u
#define HZ_MI_RQ 2u
#define HZ_MI_EXITS 4u
#define HZ_MI_CREATES 8u
#define HZ_MI_AUX 16u
#define HZ_MI_GROWING 32u
/* what a descriptor does: zeros; rows first_row .. of a source array; one element of it in every row; then the signals packed from the
 * uploaded rows, one kind each */
enum {
    HZ_MI_KIND_ZERO = 0, HZ_MI_KIND_COPY = 1, HZ_MI_KIND_BROADCAST = 2, HZ_MI_KIND_TX_COMPRESSED_DATA = 3, HZ_MI_KIND_TX_COMPRESSED_DATA_V2 = 4,
    HZ_MI_KIND_AMOUNT_F = 5, HZ_MI_KIND_FROM_IDX = 6, HZ_MI_KIND_TO_IDX = 7, HZ_MI_KIND_TO_BJJ_AY = 8, HZ_MI_KIND_TO_ETH_ADDR = 9,
    HZ_MI_KIND_MAX_NUM_BATCH = 10, HZ_MI_KIND_ON_CHAIN = 11, HZ_MI_KIND_NEW_ACCOUNT = 12, HZ_MI_KIND_RQ_OFFSET = 13, HZ_MI_KIND_RQ_V2 = 14,
    HZ_MI_KIND_RQ_TO_ETH_ADDR = 15, HZ_MI_KIND_RQ_TO_BJJ_AY = 16, HZ_MI_KIND_S = 17, HZ_MI_KIND_R8X = 18, HZ_MI_KIND_R8Y = 19,
    HZ_MI_KIND_LOAD_AMOUNT_F = 20, HZ_MI_KIND_FROM_ETH_ADDR = 21, HZ_MI_KIND_KEY_BITS = 22, HZ_MI_KINDS = 23
};
/* where a descriptor reads: nothing; array q of hz_ledger_out, as HZ_MI_SRC_OUT + q, of hz_ledger_exit_out, of hz_ledger_create_out; the
 * auxToIdx rows; the call's scalars as elements (old_last_idx, chain id, current_num_batch); fee_idxs; fee_plan_tokens; the uploaded
 * rows (hz_l1tx / hz_l2tx / hz_l2sig / hz_l2rq); from_bjj */
enum {
    HZ_MI_SRC_NONE = 0, HZ_MI_SRC_OUT = 1, HZ_MI_SRC_EXIT = 32, HZ_MI_SRC_CREATE = 40, HZ_MI_SRC_AUX_TO_IDX = 48, HZ_MI_SRC_GLOBALS = 49,
    HZ_MI_SRC_FEE_IDXS = 50, HZ_MI_SRC_FEE_PLAN_TOKENS = 51, HZ_MI_SRC_ROWS = 52, HZ_MI_SRC_KEYS = 53
};
hz_status hz_ledger_main_inputs(hz_ledger* l, const hz_ctx* ctx, uint64_t old_last_idx, void* d_packed, size_t bytes);
double hz_ledger_main_inputs_ms(const hz_ledger* l);
#define HZ_LEDGER_JOURNAL_MAX 64
hz_status hz_ledger_journal(hz_ledger* l, uint32_t depth);
hz_status hz_ledger_applied(const hz_ledger* l, uint64_t* mark);
hz_status hz_ledger_rollback(hz_ledger* l, uint64_t mark);
hz_status hz_ledger_journal_stats(const hz_ledger* l, uint32_t* depth, size_t* records, uint64_t* oldest_mark, size_t* bytes_used, size_t* bytes_reserved);
double hz_ledger_journal_ms(const hz_ledger* l);  /* device time of the capture kernels in the last apply */
double hz_ledger_rollback_ms(const hz_ledger* l); /* device time of the last rollback */
hz_status hz_ledger_plan_main_inputs(size_t n_signals, const char* const* names, const uint64_t* offsets, const uint32_t* widths, const uint64_t* flat_lens,
                                     uint64_t bytes, uint32_t n_tx, uint32_t n_levels, uint32_t max_l1_tx, uint32_t max_fee_tx, uint32_t flags,
                                     uint32_t* kind_out /* [n_signals] */, uint32_t* source_out, uint64_t* first_row_out, uint64_t* rows_out);

/* Poseidon batch: n independent permutations of width t = n_inputs + 1 (2..7). ----------------
 * `in`  : [n][t-1] canonical elements; `out`: [n] digests (state[0] after the last round).
 * If `sbox_witness` is non-NULL it receives the S-box signals (in2,in4,out per S-box, the
 * non-linear signals of circomlib's Poseidon template) as [3*(8t+R_P)][n] elements. */
hz_status hz_poseidon_batch(int32_t device, int32_t t, size_t n, const uint8_t* in, uint8_t* out, uint8_t* sbox_witness);
hz_status hz_poseidon_batch_dev(int32_t t, size_t n, const void* d_in, void* d_out, void* d_sbox_witness, void* stream);

/* Field self test (SURVEY 8a' K0): out[i] = a[i] (op) b[i] over BN254 Fr, one operation per lane, canonical operands and results.
 * No reference counterpart (the reference's field is ffiasm's Fr, tools/helpers/actions.js:207-215); used by tests/ only. */
enum { HZ_FR_ADD = 0, HZ_FR_SUB = 1, HZ_FR_MUL = 2, HZ_FR_SQR = 3, HZ_FR_INV = 4 /* inverse(0) = 0 */, HZ_FR_MULADD = 5 /* a*b + a + b */, HZ_FR_MIX = 6 /* 2a * (-b) */,
       HZ_FR_SQRT = 7 /* circomlib pointbits.circom sqrt(): the root <= (r-1)/2 of a, 0 when a is a non-residue (AySign2Ax, src/lib/utils-bjj.circom:37-58) */ };
hz_status hz_fr_ops(int32_t device, int32_t op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out);

/* Field self test on raw limbs: ONE routine of circuits_amd/csrc/fr.h per call, on operands given as 9 x 29-bit limbs exactly as the
 * routine sees them (tests/test_fr_contract.py: every routine at the edges of its stated operand range). A self test, used by tests/
 * only; no reference counterpart.
 *   operands  uint32[n_operands][n][9], plain limb arrays. NO range validation: the caller owns the routine's preconditions.
 *             An Fc operand (HZ_FRR_FROM_CANON; the exponent of HZ_FRR_POW) is 8 x u32 in words 0..7, a u64 (HZ_FRR_FROM_U64) words 0..1.
 *   out       uint32[n][9]: an Fr result as its 9 limbs; an Fc result in words 0..7 with word 8 zero; a boolean in word 0, the rest zero.
 *   form      0: the kernel is built with HZ_FR_INLINE, as every kernel of the step is; 1: built without it, so fr_mul, fr_sqr,
 *             fr_to_canon and fr_inv are the out-of-line bodies that the gadget mains call. The same kernel body otherwise.
 *   mapping   256-thread workgroups, element i runs on thread i of the launch (workgroup i / 256, wavefront (i % 256) / 64, lane
 *             i % 64) for n <= 2048 * 256; a grid-stride loop only beyond that. The tests place values on chosen lanes of chosen
 *             wavefronts through this mapping (fr_cond_sub_p_rare's and fr_inv's wave-uniform branches).
 * One kernel instantiation per op: a routine's code does not depend on the others that share the entry point.
 * Operands per op, in order -- HZ_FRR_SUB3: m a b c; HZ_FRR_SUB_A_2X: s a x; HZ_FRR_MULADD: a b s; HZ_FRR_MULADD2: a0 b0 a1 b1 s;
 * HZ_FRR_DOT1 + (N-1): a0 b0 .. a(N-1) b(N-1); HZ_FRR_DOT1_ADD + (N-1): the same and the addend; HZ_FRR_POW: a, exponent.
 * HZ_ERR_ARG for a bad op or form, an n_operands that is not the op's, or a null pointer with n > 0; n = 0 is HZ_OK. */
enum { HZ_FRR_ADD = 0, HZ_FRR_SUB, HZ_FRR_NEG, HZ_FRR_DBL, HZ_FRR_SUB_LAZY, HZ_FRR_DBL_LAZY, HZ_FRR_ADD_LAZY, HZ_FRR_SUB2_LAZY, HZ_FRR_3A_B_C_LAZY,
       HZ_FRR_SUB3, HZ_FRR_SUB_A_2X, HZ_FRR_COND_SUB_2P, HZ_FRR_COND_SUB_4P, HZ_FRR_COND_SUB_P, HZ_FRR_COND_SUB_P_RARE, HZ_FRR_IS_ZERO, HZ_FRR_EQ,
       HZ_FRR_MUL, HZ_FRR_SQR, HZ_FRR_MULADD, HZ_FRR_MULADD2, HZ_FRR_DOT1 /* .. HZ_FRR_DOT1 + 5: fr_dot<6> */, HZ_FRR_DOT1_ADD = HZ_FRR_DOT1 + 6 /* .. + 5 */,
       HZ_FRR_FROM_CANON = HZ_FRR_DOT1_ADD + 6, HZ_FRR_FROM_U64, HZ_FRR_TO_CANON, HZ_FRR_CANON_LIMBS, HZ_FRR_PACK_CANON, HZ_FRR_INV, HZ_FRR_INV_FERMAT,
       HZ_FRR_POW, HZ_FRR_COUNT };
hz_status hz_fr_raw_ops(int32_t device, int32_t op, int32_t form, size_t n, const uint32_t* operands, int32_t n_operands, uint32_t* out);

/* multi-GPU, one process per GPU (reference src/rollup-main.circom:93-99: every DecodeTx / RollupTx is
 * independent given the im* inputs). A RollupMain batch is sharded by transaction index:
 *   hz_shard_range      contiguous range of a rank
 *   hz_ctx_set_shard    this context evaluates only [first, first+count); tail != 0 on the rank that
 *                       also evaluates the fee transactions and HashInputs. count = 0 is a legal (empty) shard -- more
 *                       ranks than transactions --, count < 0 returns the context to the whole batch
 *   hz_da_export        pack the shard's per-transaction data-availability records (hz_da_record_bytes
 *                       each: L1TxFullData / L1L2TxData bits, outIdx, newExitRoot) into a device buffer --
 *                       the only data HashInputs needs from other ranks (one RCCL all_gather, ~47-330 KB)
 *   hz_da_import        write received records into this context's witness
 *   hz_witness_enqueue_tail   FeeTx + HashInputs after the imports; then hz_witness_check */
void hz_shard_range(int32_t nTx, int32_t world, int32_t rank, int32_t* first, int32_t* count);
hz_status hz_ctx_set_shard(hz_ctx* ctx, int32_t first, int32_t count, int32_t tail);
uint64_t hz_da_record_bytes(const hz_ctx* ctx);
hz_status hz_da_export(hz_ctx* ctx, void* d_buf, void* stream);
hz_status hz_da_import(hz_ctx* ctx, int32_t first, int32_t count, const void* d_buf, void* stream);
hz_status hz_witness_enqueue_tail(hz_ctx* ctx, void* stream);
/* The tail split over the ranks (SURVEY 8e "or scatter blocks back: 766 / 8"): the SHA-256 chain of HashInputs is sequential (rank 0),
 * the bit-level witness of its blocks -- 0.73 GB of the 0.76 GB the tail writes at (2048, 32) -- is independent per block given the
 * message block and the chaining value that enters it:
 *   hz_witness_enqueue_tail_chain   rank 0, after the imports: FeeTx, the message, the chain, the public output; no block witness
 *   hz_sha_blocks / hz_sha_state_bytes   number of blocks; bytes of (message blocks, chaining values): 96 B per block + 32
 *   hz_sha_export                   rank 0: that state into a device buffer (ONE broadcast, 73 KB at 766 blocks)
 *   hz_sha_expand                   any rank: take the state from the buffer (NULL on the rank that computed it) and write the
 *                                   witness of blocks [first, first + count) into this context's HashInputs section
 * Block ranges: hz_shard_range(hz_sha_blocks(ctx), world, rank, ...). The witness stays sharded: rank r holds its blocks' signals. */
hz_status hz_witness_enqueue_tail_chain(hz_ctx* ctx, void* stream);
uint64_t hz_sha_blocks(const hz_ctx* ctx);
uint64_t hz_sha_state_bytes(const hz_ctx* ctx);
hz_status hz_sha_export(hz_ctx* ctx, void* d_buf, void* stream);
hz_status hz_sha_expand(hz_ctx* ctx, int32_t first, int32_t count, const void* d_buf, void* stream);

/* The whole sharded pass inside the library, for a host in any language (the N-API addon binds it: circuit.shardStep). Counterpart of
 * the `-n` thread-per-component mode of the reference's compiled witness calculator (tools/helpers/actions.js:39-45).
 *   hz_comm_create   one per rank. transport HZ_COMM_RCCL: librccl.so is loaded with dlopen (no link-time dependency; HZ_RCCL_LIB names
 *                    another file), rank 0's ncclGetUniqueId travels over the rendezvous, ncclCommInitRank on `device`; the collectives
 *                    are ncclAllGather / ncclBroadcast on the pass's stream (xGMI). HZ_COMM_SOCKET: the two collectives staged through
 *                    host memory over the rendezvous itself (47-330 KB + 73 KB per pass: latency-sized) -- for boxes without RCCL and for
 *                    tests. rendezvous_path: a Unix socket name every rank of the node can reach (rank 0 listens on it, the others
 *                    connect, HZ_COMM_TIMEOUT_S seconds of patience, default 120); may be NULL when world == 1.
 *   hz_shard_step    one pass on `stream` (NULL: the context's own): this rank's transactions, all_gather of the data-availability records, rank 0's
 *                    imports + FeeTx + message + SHA-256 chain, broadcast of the block states, this rank's share of the block
 *                    witness. The first call shards the context (hz_ctx_set_shard with hz_shard_range(nTx, world, rank)) and
 *                    allocates the exchange buffers; every rank calls hz_witness_check afterwards. A communicator serves one context. */
typedef struct hz_comm hz_comm;
enum { HZ_COMM_RCCL = 1, HZ_COMM_SOCKET = 2 };
hz_status hz_comm_create(int32_t transport, int32_t device, int32_t rank, int32_t world, const char* rendezvous_path, hz_comm** out);
void hz_comm_destroy(hz_comm* comm);
int32_t hz_comm_rank(const hz_comm* comm);
int32_t hz_comm_world(const hz_comm* comm);
hz_status hz_shard_step(hz_ctx* ctx, hz_comm* comm, void* stream);
int32_t hz_ctx_ntx(const hz_ctx* ctx);   /* transactions per batch of a RollupMain context (0 otherwise) */

#ifdef __cplusplus
}
#endif
#endif
