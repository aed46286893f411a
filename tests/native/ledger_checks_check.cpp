// The ledger's argument checks (csrc/ledger_checks.h) built for the host: what each hz_ledger_plan_* export decides about its arguments,
// on the cases of tests/golden/ledger_arg_errors.json.gz in the line format of tests/ledger_arg_errors_common.py. Every input array lies in a
// heap block of exactly its size, so under the address sanitizer a check that reads a row it was not given, or reads on after the error
// that should have stopped it, ends the program. Output: one line per case, the status, a tab, the message ("" of a success).
//   case <export> / n <name> <hex> / a <name> null | <bytes hex> <the bytes in hex, - for none> / end
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include "../../circuits_amd/csrc/ledger_checks.h"
#include "../../circuits_amd/csrc/ledger_plan.h"
#include "../../circuits_amd/csrc/ledger_tables.h"   // ledger_wants_receiver
#include "../../circuits_amd/csrc/smt_plan.h"

static char g_err[1024];
namespace hz {
hz_status set_err(hz_status st, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return st;
}
}  // namespace hz
using namespace hz;

struct Case {
    std::string call;
    std::map<std::string, uint64_t> n;
    std::map<std::string, uint8_t*> a;   // null: a null pointer
    template <class T>
    const T* arr(const char* name) { return (const T*)a[name]; }
    ~Case() {
        for (auto& kv : a) free(kv.second);
    }
};

// the export's checks and planner, as csrc/ledger.hip runs them in front of its copies out
static hz_status run(Case& c) {
    const char* who = c.call.c_str();
    const size_t n_l1 = c.n["n_l1"], m = c.n["m"], F = c.n["F"], n_sib = c.n["n_sib"];
    const int32_t k = (int32_t)c.n["k"];
    const uint64_t first_idx = c.n["first_idx"];
    const hz_l1tx* l1 = c.arr<hz_l1tx>("l1");
    const hz_l2tx* txs = c.arr<hz_l2tx>("txs");
    const uint32_t* toks = c.arr<uint32_t>("toks");
    const uint64_t* idxs = c.arr<uint64_t>("idxs");
    LedgerPlan p;
    if (c.call == "hz_ledger_plan_l2") {
        if (hz_status e = ledger_check_k(who, k)) return e;
        return ledger_check_plan(who, m, txs, F, toks, idxs, 1ull << k, first_idx, p);
    }
    if (c.call == "hz_ledger_plan_batch") {
        if (hz_status e = ledger_check_plan_rows(who, k, first_idx, false, 0, n_l1, l1, m, txs, F, toks, idxs, p)) return e;
        ledger_plan_batch(n_l1, l1, m, txs, F, toks, idxs, p);
        return HZ_OK;
    }
    if (c.call == "hz_ledger_plan_exits") {
        if (hz_status e = ledger_check_plan_rows(who, k, first_idx, true, n_sib, n_l1, l1, m, txs, F, toks, idxs, p)) return e;
        ledger_plan_exits(n_l1, l1, m, txs, F, toks, idxs, p);
        SmtShape sh;
        sh.begin();
        for (size_t x = 0; x < p.exit_row.size(); x++)
            if (sh.add(p.exit_key[x], (uint32_t)n_sib) != SMT_PLAN_OK)
                return set_err(HZ_ERR_ARG, "%s: op %zu (key %llu) would have its leaf at depth >= n_sib = %zu: SMTProcessor(%zu) cannot express it", who, x,
                               (unsigned long long)p.exit_key[x], n_sib, n_sib);
        return HZ_OK;
    }
    if (c.call == "hz_ledger_plan_creates") {
        LedgerRows r;
        return ledger_check_plan_creates(who, LedgerShape{c.n["growing"] != 0, c.n["capacity"], first_idx, c.n["size"], 0}, n_l1, l1, c.arr<uint8_t>("from_bjj"), m, txs, F, toks,
                                         idxs, r);
    }
    if (c.call == "hz_ledger_plan_atomic") return ledger_check_plan_atomic(who, n_l1, m, txs, c.arr<hz_l2sig>("sigs"), c.arr<hz_l2rq>("rq"));
    if (c.call == "hz_ledger_plan_select") {
        const uint64_t* aux = c.arr<uint64_t>("aux");
        if (hz_status e = select_check_plan(who, n_l1, l1, m, txs, c.arr<int32_t>("partner"))) return e;
        std::vector<hz_l2tx> eff(txs, txs + m);
        for (size_t i = 0; i < m; i++)
            if (aux && ledger_wants_receiver(eff[i])) eff[i].to_idx = aux[i];
        SelectPlan sp;
        return select_plan(who, n_l1, l1, m, eff.data(), p, sp);
    }
    return set_err(HZ_ERR_ARG, "%s: not an export this program knows", who);
}

int main() {
    std::string line;
    Case* c = nullptr;
    size_t cases = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string tag, name, word;
        in >> tag;
        if (tag == "case") {
            c = new Case;
            in >> c->call;
        } else if (tag == "n") {
            in >> name >> word;
            c->n[name] = strtoull(word.c_str(), nullptr, 16);
        } else if (tag == "a") {
            in >> name >> word;
            uint8_t* block = nullptr;
            if (word != "null") {
                const size_t bytes = strtoull(word.c_str(), nullptr, 16);
                in >> word;
                block = (uint8_t*)malloc(bytes);   // exactly the array: a byte beyond it is the sanitizer's
                for (size_t i = 0; i < bytes; i++) {
                    const char hex[3] = {word[2 * i], word[2 * i + 1], 0};
                    block[i] = (uint8_t)strtoul(hex, nullptr, 16);
                }
            }
            c->a[name] = block;
        } else if (tag == "end") {
            g_err[0] = 0;
            const hz_status st = run(*c);
            printf("%d\t%s\n", (int)st, st ? g_err : "");
            delete c;
            c = nullptr;
            cases++;
        }
    }
    fprintf(stderr, "cases=%zu\n", cases);
    return 0;
}
