// hz_smt: the host planner of the sparse device-resident Merkle tree (smt_tree.hip). Integers only -- no field arithmetic, no hash, no
// HIP include -- so it runs, and is tested, without a device (hz_smt_plan).
//
// circomlib's tree is a function of its key set: slot (d, p) (depth d, p = key mod 2^d, key bits LSB first) with c keys below it is
// empty (c = 0), a leaf whose hash does not depend on d (c = 1), or an internal node over (d + 1, p) and (d + 1, p + 2^d) (c >= 2). The
// slot table is kept in the one form in which a walk needs no lookup: the slots with c >= 2 are numbered (their number is their place
// in the device's node pool) and hold what their two child slots are -- nothing, leaf number l (c = 1: the slot's only key is
// leaf_key[l], its place in the device's leaf and value pools l), or node number n. A reference is an int32: 0 empty, n + 1 node n,
// -(l + 1) leaf l.
//
// One call is m ORDERED operations. Operation j on key K (insert if absent, update if present) puts K's leaf at D_j, the shallowest
// depth where K is alone afterwards, and makes VERSION j of the D_j internal slots on its path. Version j of the slot at depth d is the
// hash of its own child (leaf hash j when D_j = d + 1, else version j at d + 1) and the OTHER child as it stands at time j: nothing, a
// leaf (the leaf hash of the latest earlier operation of this call on that key, else the resident one), or a node (its latest earlier
// version of this call, else the resident one). The planner walks the operations in order, keeps the shape up to date and writes down
// where each of those two inputs lies -- a SOURCE: kind and index --, per depth and compacted, so that the device runs one launch per
// depth whatever m is. Every change is logged; rollback() undoes a call that is refused or fails later.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace hz {

// where a 32-byte element lies: kind (the buffer) in the top three bits, index in the low 29
enum : uint32_t {
    SMT_ZERO = 0,    // the field's zero (an empty slot; the old value of an insert into an empty slot)
    SMT_CALL_LH = 1, // leaf hash of operation [index] of this call
    SMT_LEAF = 2,    // resident leaf hash of leaf [index]
    SMT_VER = 3,     // node version [index] of this call (planner: depth << 20 | place in that depth's list; flat(): the global place)
    SMT_NODE = 4,    // resident digest of node [index]
    SMT_CALL_LV = 5, // value (state hash) of operation [index] of this call
    SMT_VALUE = 6,   // resident value of leaf [index]
    SMT_KINDS = 7
};
#define HZ_SMT_MAX_DEPTH 64
#define HZ_SMT_KEY_BITS 48
#define HZ_SMT_POOL_CAP (1u << 28)   // nodes, and leaves, a tree can hold: an index fits a source with room to spare

inline uint32_t smt_src(uint32_t kind, uint32_t index) { return kind << 29 | index; }

// one hash of a level launch: version (depth, place) = Poseidon(own, other), swapped when the path goes right
struct SmtLevelOp {
    uint32_t own, other;
    uint32_t meta;   // bits 0-15 operation j, 16-21 depth d, 30: `other` is sibling d of operation j's proof, 31: the path goes right at d
};

enum SmtPlanError { SMT_PLAN_OK = 0, SMT_PLAN_KEY = 1 /* key >= 2^48 */, SMT_PLAN_DEPTH = 2 /* leaf at depth >= n_sib */, SMT_PLAN_FULL = 3 };

struct SmtShape {
    // ---- the tree ----
    int32_t root = 0;
    std::vector<int32_t> child;      // [2 * nodes]
    std::vector<uint64_t> leaf_key;  // [leaves]
    // ---- the call being planned ----
    std::vector<int32_t> node_ver;   // [nodes]: depth << 20 | place of the node's latest version in this call, -1: none yet
    std::vector<int32_t> leaf_op;    // [leaves]: latest operation of this call on the leaf, -1: none yet
    std::vector<uint32_t> touched_nodes, touched_leaves;
    std::vector<SmtLevelOp> level[HZ_SMT_MAX_DEPTH];
    std::vector<uint32_t> root_src;  // [m + 1]: the root before operation j (so [j + 1]: after it)
    std::vector<uint32_t> old_value_src, depth;
    std::vector<uint64_t> old_key;
    std::vector<uint8_t> is_old0, fnc;
    uint32_t max_depth = 0;
    // undo log: (place in `child`, or -1 for the root; the reference it held)
    struct Undo { int64_t at; int32_t ref; };
    std::vector<Undo> undo;
    size_t nodes0 = 0, leaves0 = 0;

    size_t nodes() const { return child.size() / 2; }
    size_t leaves() const { return leaf_key.size(); }

    void clear() {
        root = 0;
        child.clear();
        leaf_key.clear();
        node_ver.clear();
        leaf_op.clear();
        begin();
    }

    // source of what a reference stands for at this point of the call
    uint32_t hash_src(int32_t ref) const {
        if (ref == 0) return smt_src(SMT_ZERO, 0);
        if (ref < 0) {
            const uint32_t l = (uint32_t)(-ref - 1);
            return leaf_op[l] >= 0 ? smt_src(SMT_CALL_LH, (uint32_t)leaf_op[l]) : smt_src(SMT_LEAF, l);
        }
        const uint32_t n = (uint32_t)(ref - 1);
        return node_ver[n] >= 0 ? smt_src(SMT_VER, (uint32_t)node_ver[n]) : smt_src(SMT_NODE, n);
    }
    uint32_t value_src(uint32_t l) const { return leaf_op[l] >= 0 ? smt_src(SMT_CALL_LV, (uint32_t)leaf_op[l]) : smt_src(SMT_VALUE, l); }

    void begin() {
        for (auto& l : level) l.clear();
        root_src.assign(1, hash_src(root));
        old_value_src.clear();
        depth.clear();
        old_key.clear();
        is_old0.clear();
        fnc.clear();
        undo.clear();
        touched_nodes.clear();
        touched_leaves.clear();
        max_depth = 0;
        nodes0 = nodes();
        leaves0 = leaves();
    }

    void set_ref(int64_t at, int32_t ref) {
        int32_t& r = at < 0 ? root : child[(size_t)at];
        undo.push_back({at, r});
        r = ref;
    }

    // operation j = number of operations planned so far. Nothing changes when it is refused.
    SmtPlanError add(uint64_t key, uint32_t n_sib) {
        if (key >> HZ_SMT_KEY_BITS) return SMT_PLAN_KEY;
        const uint32_t j = (uint32_t)depth.size();
        uint32_t path[HZ_SMT_MAX_DEPTH + 1];
        int32_t ref = root;
        int64_t at = -1;   // where `ref` is held
        uint32_t f = 0;    // the find depth: where the walk ends
        while (ref > 0) {
            if (f >= n_sib) return SMT_PLAN_DEPTH;
            path[f] = (uint32_t)(ref - 1);
            at = (int64_t)path[f] * 2 + (int64_t)((key >> f) & 1);
            ref = child[(size_t)at];
            f++;
        }
        uint32_t D = f, leaf;
        if (ref < 0 && leaf_key[(size_t)(-ref - 1)] == key) {   // update
            if (D >= n_sib) return SMT_PLAN_DEPTH;
            leaf = (uint32_t)(-ref - 1);
            fnc.push_back(0);
            is_old0.push_back(0);
            old_key.push_back(key);
            old_value_src.push_back(value_src(leaf));
        } else {
            uint32_t e = f;   // meeting another leaf: both move below the first bit at or past f in which the keys differ
            if (ref < 0) {
                const uint64_t x = (key ^ leaf_key[(size_t)(-ref - 1)]) >> f;
                while (!((x >> (e - f)) & 1)) e++;
                D = e + 1;
            }
            if (D >= n_sib) return SMT_PLAN_DEPTH;
            if (leaves() >= HZ_SMT_POOL_CAP || nodes() + (D - f) > HZ_SMT_POOL_CAP) return SMT_PLAN_FULL;
            leaf = (uint32_t)leaves();
            leaf_key.push_back(key);
            leaf_op.push_back(-1);
            fnc.push_back(1);
            if (ref == 0) {
                is_old0.push_back(1);
                old_key.push_back(key);
                old_value_src.push_back(smt_src(SMT_ZERO, 0));
                set_ref(at, -(int32_t)leaf - 1);
            } else {
                const uint32_t met = (uint32_t)(-ref - 1);
                is_old0.push_back(0);
                old_key.push_back(leaf_key[met]);
                old_value_src.push_back(value_src(met));
                for (uint32_t d = f; d <= e; d++) {   // new nodes at depths f .. e; the two leaves hang below the one at e
                    const uint32_t n = (uint32_t)nodes();
                    child.push_back(0);
                    child.push_back(0);
                    node_ver.push_back(-1);
                    path[d] = n;
                    set_ref(at, (int32_t)n + 1);
                    at = (int64_t)n * 2 + (int64_t)((key >> d) & 1);
                }
                set_ref(at, -(int32_t)leaf - 1);
                set_ref(at ^ 1, ref);
            }
        }
        depth.push_back(D);
        if (D > max_depth) max_depth = D;
        uint32_t own = smt_src(SMT_CALL_LH, j);
        for (uint32_t d = D; d-- > 0;) {
            const uint32_t n = path[d], right = (uint32_t)((key >> d) & 1);
            const uint32_t place = (uint32_t)level[d].size();
            level[d].push_back({own, hash_src(child[(size_t)n * 2 + (right ^ 1)]), j | d << 16 | (d < f ? 1u << 30 : 0u) | right << 31});
            if (node_ver[n] < 0) touched_nodes.push_back(n);
            node_ver[n] = (int32_t)(d << 20 | place);
            own = smt_src(SMT_VER, d << 20 | place);
        }
        if (leaf_op[leaf] < 0) touched_leaves.push_back(leaf);
        leaf_op[leaf] = (int32_t)j;
        root_src.push_back(own);
        return SMT_PLAN_OK;
    }

    // the planned call as the device takes it: the level lists lie behind each other in one array, depth d's at first[d] (firsts()), and
    // a version source (depth, place in that depth's list) becomes the global place first[depth] + place
    uint32_t global_ver(uint32_t packed, const uint32_t* first) const { return first[packed >> 20] + (packed & 0xFFFFFu); }
    uint32_t flat_src(uint32_t s, const uint32_t* first) const {
        return s >> 29 == SMT_VER ? smt_src(SMT_VER, global_ver(s & 0x1FFFFFFFu, first)) : s;
    }
    size_t versions() const {
        size_t n = 0;
        for (uint32_t d = 0; d < max_depth; d++) n += level[d].size();
        return n;
    }
    void firsts(uint32_t* first) const {
        uint32_t n = 0;
        for (uint32_t d = 0; d < HZ_SMT_MAX_DEPTH; d++) {
            first[d] = n;
            n += d < max_depth ? (uint32_t)level[d].size() : 0u;
        }
    }

    // the call stands: forget the per-call marks
    void commit() {
        for (uint32_t n : touched_nodes) node_ver[n] = -1;
        for (uint32_t l : touched_leaves) leaf_op[l] = -1;
        begin();
    }

    // the call did not happen
    void rollback() {
        for (uint32_t n : touched_nodes) node_ver[n] = -1;
        for (uint32_t l : touched_leaves) leaf_op[l] = -1;
        for (size_t i = undo.size(); i-- > 0;) {
            if (undo[i].at < 0) root = undo[i].ref;
            else if ((size_t)undo[i].at < nodes0 * 2) child[(size_t)undo[i].at] = undo[i].ref;
        }
        child.resize(nodes0 * 2);
        node_ver.resize(nodes0);
        leaf_key.resize(leaves0);
        leaf_op.resize(leaves0);
        begin();
    }

    // what a call that stands changed of the shape, for an owner that may want the call undone later (ledger_journal.h): the references it
    // replaced in slots the tree already had, and the counts it found
    struct UndoLog {
        std::vector<Undo> undo;
        size_t nodes0 = 0, leaves0 = 0;
    };

    // commit(), but hand me the undo
    void commit_undo(UndoLog& out) {
        out.undo.clear();
        for (const Undo& u : undo)
            if (u.at < 0 || (size_t)u.at < nodes0 * 2) out.undo.push_back(u);
        out.nodes0 = nodes0;
        out.leaves0 = leaves0;
        commit();
    }

    // revert this undo: the shape as it was before the call that handed it out. No call is in progress, and every later call has been
    // reverted already (newest first): the entries the call added are the pools' last
    void revert(const UndoLog& u) {
        for (size_t i = u.undo.size(); i-- > 0;) {
            if (u.undo[i].at < 0) root = u.undo[i].ref;
            else child[(size_t)u.undo[i].at] = u.undo[i].ref;
        }
        child.resize(u.nodes0 * 2);
        node_ver.resize(u.nodes0);
        leaf_key.resize(u.leaves0);
        leaf_op.resize(u.leaves0);
        begin();
    }

    // a walk for a proof against the resident tree (no call in progress): the find depth, what the walk met (0 nothing, else a leaf
    // reference), and the sibling sources of depths 0 .. f - 1 in sib[]
    uint32_t find(uint64_t key, int32_t* met, uint32_t* sib) const {
        int32_t ref = root;
        uint32_t f = 0;
        while (ref > 0) {
            const size_t n = (size_t)(ref - 1), bit = (size_t)((key >> f) & 1);
            if (sib && f < HZ_SMT_MAX_DEPTH) sib[f] = hash_src(child[n * 2 + (bit ^ 1)]);
            ref = child[n * 2 + bit];
            f++;
        }
        *met = ref;
        return f;
    }
};

}  // namespace hz
