// Exact endgames in the search plan (alphazero_amd/csrc/az_search_plan.h) without a GPU, for tests/test_search_plan_exact.py:
//   search_plan_exact refusal EVALUATOR SYM SYMR LEAF_BATCH GM CAP FORCED   the mode that refuses, or "served"
//   search_plan_exact arg MAX_EMPTIES                                      1 where the setter takes the value
//   search_plan_exact plan EXACT CAP FORCED GM K N_SIM                     the family, L and launches, then one line per launch
//   search_plan_exact keycmp EXACT_A EXACT_B N_SIM ROWS G0 G1              == or != : the graph keys of two plain searches
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "az_search_plan.h"

static SearchMode mode(int exact, bool cap, bool forced, int gm, int K) {
    SearchMode m = {false, gm, K, false, cap, forced, exact};
    return m;
}

int main(int argc, char **argv) {
    const auto arg = [&](int i) { return atoi(argv[i]); };
    if (argc == 9 && !strcmp(argv[1], "refusal")) {
        const char *why = exact_endgame_refusal(arg(2), arg(3) != 0, arg(4) != 0, arg(5), arg(6), arg(7) != 0, arg(8) != 0);
        printf("%s\n", why ? why : "served");
    } else if (argc == 3 && !strcmp(argv[1], "arg")) {
        printf("%d %d\n", exact_endgame_ok(arg(2)) ? 1 : 0, AZ_EXACT_MAX_EMPTIES);
    } else if (argc == 8 && !strcmp(argv[1], "plan")) {
        const SearchMode m = mode(arg(2), arg(3) != 0, arg(4) != 0, arg(5), arg(6));
        const SearchPlan p = plan_search(m, arg(7));
        printf("%s %d %d %d\n", search_family_name(p.family), p.L, p.launches, p.root_pass);
        for (int t = 0; t < p.launches; ++t) {
            const StepArgs a = plan_step(p, arg(7), m.K, t);
            printf("%d %d %d %d\n", a.backup, a.select, a.t, a.ctr);
        }
    } else if (argc == 8 && !strcmp(argv[1], "keycmp")) {
        const SearchKey a = search_key(plan_search(mode(arg(2), false, false, 0, 1), arg(4)), arg(4), arg(5), arg(6), arg(7));
        const SearchKey b = search_key(plan_search(mode(arg(3), false, false, 0, 1), arg(4)), arg(4), arg(5), arg(6), arg(7));
        printf("%s\n", a == b ? "==" : "!=");
    } else {
        fprintf(stderr, "usage: %s refusal ... | arg E | plan EXACT CAP FORCED GM K N_SIM | keycmp EA EB N_SIM ROWS G0 G1\n", argv[0]);
        return 2;
    }
    return 0;
}
