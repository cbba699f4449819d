// The PUCT exploration settings in the search plan (alphazero_amd/csrc/az_search_plan.h) without a GPU, for
// tests/test_search_plan_puct.py:
//   search_plan_puct refusal EVALUATOR SYM SYMR LEAF_BATCH GM CAP FORCED EXACT PROOF   the mode that refuses, or "served"
//   search_plan_puct plan PUCT PROOF EXACT CAP FORCED GM K ROLLOUT N_SIM              the family, L, launches, root pass and the exact
//                                                                                     property, then one line per launch
//   search_plan_puct keycmp PUCT_A PUCT_B N_SIM ROWS G0 G1                            == or != : the graph keys of two plain searches
//   search_plan_puct ranges C_INIT C_BASE FPU                                         c_init ok, c_base ok, fpu ok, neutral
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "az_search_plan.h"

static SearchMode mode(bool puct, bool proof, int exact, bool cap, bool forced, int gm, int K, bool rollout) {
    SearchMode m = {rollout, gm, K, false, cap, forced, exact, proof, puct};
    return m;
}

int main(int argc, char **argv) {
    const auto arg = [&](int i) { return atoi(argv[i]); };
    if (argc == 11 && !strcmp(argv[1], "refusal")) {
        const char *why = puct_refusal(arg(2), arg(3) != 0, arg(4) != 0, arg(5), arg(6), arg(7) != 0, arg(8) != 0, arg(9), arg(10) != 0);
        printf("%s\n", why ? why : "served");
    } else if (argc == 11 && !strcmp(argv[1], "plan")) {
        const SearchMode m = mode(arg(2) != 0, arg(3) != 0, arg(4), arg(5) != 0, arg(6) != 0, arg(7), arg(8), arg(9) != 0);
        const SearchPlan p = plan_search(m, arg(10));
        printf("%s %d %d %d %d\n", search_family_name(p.family), p.L, p.launches, p.root_pass, p.exact);
        for (int t = 0; t < p.launches; ++t) {
            const StepArgs a = plan_step(p, arg(10), m.K, t);
            printf("%d %d %d %d\n", a.backup, a.select, a.t, a.ctr);
        }
    } else if (argc == 8 && !strcmp(argv[1], "keycmp")) {
        const SearchKey a = search_key(plan_search(mode(arg(2) != 0, false, 0, false, false, 0, 1, false), arg(4)), arg(4), arg(5), arg(6), arg(7));
        const SearchKey b = search_key(plan_search(mode(arg(3) != 0, false, 0, false, false, 0, 1, false), arg(4)), arg(4), arg(5), arg(6), arg(7));
        printf("%s\n", a == b ? "==" : "!=");
    } else if (argc == 5 && !strcmp(argv[1], "ranges")) {
        const double c_init = atof(argv[2]), c_base = atof(argv[3]), fpu = atof(argv[4]);
        printf("%d %d %d %d\n", puct_c_init_ok(c_init), puct_c_base_ok(c_base), puct_fpu_ok(fpu), puct_neutral(c_init, c_base, fpu));
    } else {
        fprintf(stderr, "usage: %s refusal ... | plan PUCT PROOF EXACT CAP FORCED GM K ROLLOUT N_SIM | keycmp PA PB N_SIM ROWS G0 G1 | ranges C_INIT C_BASE FPU\n", argv[0]);
        return 2;
    }
    return 0;
}
