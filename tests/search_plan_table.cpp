// Prints a search's launch plan (alphazero_amd/csrc/az_search_plan.h) without a GPU, for tests/test_search_plan_host.py:
//   search_plan_table plan ROLLOUT GM K FULL CAP FORCED N_SIM   the launch sequence, in enqueue_search's order, one line per launch:
//       plan <family> full=F root_pass=R L=.. launches=..
//       kernel <name>                                           (the root pass: k_root_prep, k_root_init)
//       step <family><B,S> <the kernel's integer arguments; g0 g1 for the chain's slot range>
//       forward ctr=.. step=.. kt=..
//   search_plan_table cap W K ACTIVE        search_batch_cap, then quantised_cap of it
//   search_plan_table range G N             group_range of every group
//   search_plan_table auto EVALUATOR GAME H W G
//   search_plan_table locksteps N M K       gumbel_locksteps
//   search_plan_table keycmp A B            == < or >: the graph keys of two searches, each ROLLOUT GM K FULL CAP FORCED N_SIM ROWS G0 G1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "az_search_plan.h"

static void print_plan(const SearchMode &m, int n_sim) {
    const SearchPlan p = plan_search(m, n_sim);
    const char *name = search_family_name(p.family);
    printf("plan %s full=%d root_pass=%d L=%d launches=%d\n", name, p.full, p.root_pass, p.L, p.launches);
    if (p.root_pass) printf("kernel k_root_prep\nforward ctr=2 step=-1 kt=0\nkernel k_root_init\n");
    for (int t = 0; t < p.launches; ++t) {
        const StepArgs a = plan_step(p, n_sim, m.K, t);
        switch (p.family) {
            case SF_ROLLOUT: printf("step %s %d\n", name, a.t); break;
            case SF_STEP_MULTI: printf("step %s<%d,%d> %d %d %d\n", name, a.backup, a.select, a.t, a.kb, a.kt); break;
            case SF_STEP_GUMBEL: printf("step %s<%d,%d> %d %d g0 g1\n", name, a.backup, a.select, a.t, n_sim); break;
            case SF_STEP_GUMBEL_MULTI: printf("step %s<%d,%d> %d %d\n", name, a.backup, a.select, a.t, n_sim); break;
            default: printf("step %s<%d,%d> %d g0 g1\n", name, a.backup, a.select, a.t); break;
        }
        if (a.select) printf("forward ctr=%d step=%d kt=%d\n", a.ctr, a.t, a.kt);
    }
}

// ROLLOUT GM K FULL CAP FORCED N_SIM ROWS G0 G1 from argv[i] on
static SearchKey key_of(char **argv, int i) {
    const auto arg = [&](int j) { return atoi(argv[i + j]); };
    const SearchMode m = {arg(0) != 0, arg(1), arg(2), arg(3) != 0, arg(4) != 0, arg(5) != 0};
    return search_key(plan_search(m, arg(6)), arg(6), arg(7), arg(8), arg(9));
}

int main(int argc, char **argv) {
    const auto arg = [&](int i) { return atoi(argv[i]); };
    if (argc == 9 && !strcmp(argv[1], "plan")) {
        print_plan(SearchMode{arg(2) != 0, arg(3), arg(4), arg(5) != 0, arg(6) != 0, arg(7) != 0}, arg(8));
    } else if (argc == 5 && !strcmp(argv[1], "cap")) {
        const int cap = search_batch_cap(arg(2), arg(3), arg(4));
        printf("%d %d\n", cap, quantised_cap(arg(2) * arg(3), cap));
    } else if (argc == 4 && !strcmp(argv[1], "range")) {
        for (int i = 0; i < arg(3); ++i) {
            int g0 = -1, g1 = -1;
            group_range(arg(2), i, arg(3), &g0, &g1);
            printf("%d %d\n", g0, g1);
        }
    } else if (argc == 7 && !strcmp(argv[1], "auto")) {
        printf("%d\n", groups_auto(arg(2), arg(3), arg(4), arg(5), arg(6)));
    } else if (argc == 5 && !strcmp(argv[1], "locksteps")) {
        printf("%d\n", gumbel_locksteps(arg(2), arg(3), arg(4)));
    } else if (argc == 22 && !strcmp(argv[1], "keycmp")) {
        const SearchKey a = key_of(argv, 2), b = key_of(argv, 12);
        printf("%s\n", a == b ? "==" : (a < b ? "<" : ">"));
    } else {
        fprintf(stderr, "usage: %s plan ROLLOUT GM K FULL CAP FORCED N_SIM | cap W K ACTIVE | range G N | auto EVALUATOR GAME H W G | locksteps N M K | keycmp A B\n", argv[0]);
        return 2;
    }
    return 0;
}
