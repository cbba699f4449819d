// The rule of the heads inside the search step kernel (alphazero_amd/csrc/az_search_plan.h: step_heads_*) without a GPU, for
// tests/test_search_plan_step_heads.py:
//   step_heads_table rule REQUEST EVALUATOR GAME H W G PLAIN SHAPE PROFILED   step_heads_in_force, then step_heads_auto and step_heads_served
//   step_heads_table family CAP FORCED EXACT PROOF PUCT GM K                  the kernel family plan_search gives the mode (the form is
//                                                                             launched from k_step's family alone)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "az_search_plan.h"

int main(int argc, char **argv) {
    const auto arg = [&](int i) { return atoi(argv[i]); };
    if (argc == 11 && !strcmp(argv[1], "rule")) {
        printf("%d %d %d\n", step_heads_in_force(arg(2), arg(3), arg(4), arg(5), arg(6), arg(7), arg(8) != 0, arg(9) != 0, arg(10) != 0),
               step_heads_auto(arg(3), arg(4), arg(5), arg(6), arg(7)), step_heads_served(arg(3), arg(8) != 0, arg(9) != 0, arg(10) != 0));
    } else if (argc == 9 && !strcmp(argv[1], "family")) {
        const SearchMode m = {false, arg(7), arg(8), false, arg(2) != 0, arg(3) != 0, arg(4), arg(5) != 0, arg(6) != 0};
        printf("%s\n", search_family_name(plan_search(m, 8).family));
    } else {
        fprintf(stderr, "usage: %s rule REQUEST EVALUATOR GAME H W G PLAIN SHAPE PROFILED | family CAP FORCED EXACT PROOF PUCT GM K\n", argv[0]);
        return 2;
    }
    return 0;
}
