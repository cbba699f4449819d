// Proof backup in the search plan (alphazero_amd/csrc/az_search_plan.h) without a GPU, for tests/test_search_plan_proof.py:
//   search_plan_proof refusal EVALUATOR SYM SYMR LEAF_BATCH GM CAP FORCED   the mode that refuses, or "served"
//   search_plan_proof plan PROOF EXACT CAP FORCED GM K N_SIM               the family, L, launches, root pass and the exact property,
//                                                                          then one line per launch
//   search_plan_proof keycmp PROOF_A EXACT_A PROOF_B EXACT_B N_SIM ROWS G0 G1   == or != : the graph keys of two searches
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "az_search_plan.h"

static SearchMode mode(bool proof, int exact, bool cap, bool forced, int gm, int K) {
    SearchMode m = {false, gm, K, false, cap, forced, exact, proof};
    return m;
}

int main(int argc, char **argv) {
    const auto arg = [&](int i) { return atoi(argv[i]); };
    if (argc == 9 && !strcmp(argv[1], "refusal")) {
        const char *why = proof_backup_refusal(arg(2), arg(3) != 0, arg(4) != 0, arg(5), arg(6), arg(7) != 0, arg(8) != 0);
        printf("%s\n", why ? why : "served");
    } else if (argc == 9 && !strcmp(argv[1], "plan")) {
        const SearchMode m = mode(arg(2) != 0, arg(3), arg(4) != 0, arg(5) != 0, arg(6), arg(7));
        const SearchPlan p = plan_search(m, arg(8));
        printf("%s %d %d %d %d\n", search_family_name(p.family), p.L, p.launches, p.root_pass, p.exact);
        for (int t = 0; t < p.launches; ++t) {
            const StepArgs a = plan_step(p, arg(8), m.K, t);
            printf("%d %d %d %d\n", a.backup, a.select, a.t, a.ctr);
        }
    } else if (argc == 10 && !strcmp(argv[1], "keycmp")) {
        const SearchKey a = search_key(plan_search(mode(arg(2) != 0, arg(3), false, false, 0, 1), arg(6)), arg(6), arg(7), arg(8), arg(9));
        const SearchKey b = search_key(plan_search(mode(arg(4) != 0, arg(5), false, false, 0, 1), arg(6)), arg(6), arg(7), arg(8), arg(9));
        printf("%s\n", a == b ? "==" : "!=");
    } else {
        fprintf(stderr, "usage: %s refusal ... | plan PROOF EXACT CAP FORCED GM K N_SIM | keycmp PA EA PB EB N_SIM ROWS G0 G1\n", argv[0]);
        return 2;
    }
    return 0;
}
