// The leaf evaluation cache's rule and key arithmetic (alphazero_amd/csrc/az_search_plan.h) without a GPU, for
// tests/test_search_plan_eval_cache.py:
//   eval_cache_table rule REQUEST EVALUATOR GAME H W G BEYOND PROFILED   eval_cache_in_force, then eval_cache_auto and eval_cache_served
//   eval_cache_table args CAPACITY LIMIT                                 ec_capacity_ok ec_limit_ok
//   eval_cache_table key P1 M1 PLAYER CAPACITY LIMIT                     hash, the AZ_EC_PROBE buckets, in-limit (P1 / M1 in hex)
//   eval_cache_table tag HASH SERIAL SIM                                 stamp, tag (hex), and the two fields read back
//   eval_cache_table row ENTRY                                           the negative row, whether it reads as an entry, the entry read back
//   eval_cache_table stride A
//   eval_cache_table play CAPACITY LIMIT N SEED   a host model of one group's table with the kernels' lookup (ec_lookup_grp: hits first,
//       then a claim of the first free probed entry; no eviction) over N draws from a small pool of random positions, one "kernel" of 8
//       lookups per stamp; every hit is checked against a plain map.  Prints lookups, hits, claims, misses without room, out of limit,
//       and the draws of at most LIMIT stones counted cell by cell.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <tuple>
#include <vector>

#include "az_search_plan.h"

struct Entry { uint64_t tag, p1, m1; int player; int payload; };

static uint64_t rng_state;
static uint64_t rng() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int play(int capacity, int limit, int n, int seed) {
    rng_state = (uint64_t)seed;
    std::vector<Entry> table((size_t)capacity, Entry{0, 0, 0, 0, 0});
    std::map<std::tuple<uint64_t, uint64_t, int>, int> truth;  // position -> the payload its first evaluation produced
    std::vector<std::tuple<uint64_t, uint64_t, int>> pool;
    for (int i = 0; i < 64; ++i) {  // positions of 4 .. 20 stones, both sides to move
        uint64_t occ = 0;
        const int k = 4 + (int)(rng() % 17);
        while (__builtin_popcountll(occ) < k) occ |= 1ull << (rng() % 64);
        const uint64_t p1 = occ & rng();
        pool.push_back(std::make_tuple(p1, occ & ~p1, (rng() & 1) ? 1 : -1));
    }
    long lookups = 0, hits = 0, claims = 0, no_room = 0, out = 0, small = 0;  // small: draws of at most `limit` stones, counted cell by cell
    uint32_t serial = 0;
    std::vector<std::pair<int, int>> pending;  // (entry, payload) of the claims of the previous kernel: written by the next one's backup
    for (int done = 0, sim = 0; done < n; ++sim) {
        if (sim == 5) { serial = ec_stamp(serial, sim); sim = 0; }  // the ply's last backup advances the serial word
        const uint32_t stamp = ec_stamp(serial, sim);
        for (auto &pe : pending) table[(size_t)pe.first].payload = pe.second;
        pending.clear();
        for (int s = 0; s < 8 && done < n; ++s, ++done) {
            const auto &pos = pool[rng() % pool.size()];
            const uint64_t p1 = std::get<0>(pos), m1 = std::get<1>(pos);
            const int player = std::get<2>(pos);
            ++lookups;
            int cells = 0;
            for (int c = 0; c < 64; ++c) cells += (int)(((p1 | m1) >> c) & 1);
            if (cells <= limit) ++small;
            if (!truth.count(pos)) truth[pos] = (int)truth.size() + 1;
            if (!ec_in_limit(p1, m1, limit)) { ++out; continue; }
            const uint32_t h = ec_hash(p1, m1, player);
            int hit = -1, now = 0, free_at = -1;
            for (int j = AZ_EC_PROBE - 1; j >= 0; --j) {  // descending: the lowest probe wins, as __ffs of the ballots does
                const uint32_t b = ec_bucket(h, j, (uint32_t)capacity);
                if (b >= (uint32_t)capacity) { fprintf(stderr, "bucket %u out of %d\n", b, capacity); return 1; }
                const Entry &e = table[b];
                const bool same = e.tag != 0 && ec_tag_hash(e.tag) == h, older = ec_tag_stamp(e.tag) < stamp;
                if (same && older && e.p1 == p1 && e.m1 == m1 && e.player == player) hit = (int)b;
                if (same && !older) now = 1;
                if (e.tag == 0) free_at = (int)b;
            }
            if (hit >= 0) {
                const int row = ec_row_of_entry(hit);
                if (!ec_row_is_entry(row) || ec_entry_of_row(row) != hit) { fprintf(stderr, "row encoding\n"); return 1; }
                if (table[(size_t)hit].payload != truth[pos]) { fprintf(stderr, "wrong hit: entry %d\n", hit); return 1; }
                ++hits;
            } else if (!now && free_at >= 0) {
                Entry &e = table[(size_t)free_at];
                e.tag = ec_tag(h, stamp); e.p1 = p1; e.m1 = m1; e.player = player;
                pending.push_back(std::make_pair(free_at, truth[pos]));
                ++claims;
            } else {
                ++no_room;
            }
        }
    }
    printf("%ld %ld %ld %ld %ld %ld\n", lookups, hits, claims, no_room, out, small);
    return 0;
}

int main(int argc, char **argv) {
    const auto arg = [&](int i) { return atoi(argv[i]); };
    const auto hex = [&](int i) { return (uint64_t)strtoull(argv[i], nullptr, 16); };
    if (argc == 10 && !strcmp(argv[1], "rule")) {
        printf("%d %d %d\n", eval_cache_in_force(arg(2), arg(3), arg(4), arg(5), arg(6), arg(7), arg(8) != 0, arg(9) != 0),
               eval_cache_auto(arg(3), arg(4), arg(5), arg(6), arg(7)), eval_cache_served(arg(3), arg(8) != 0, arg(9) != 0));
    } else if (argc == 4 && !strcmp(argv[1], "args")) {
        printf("%d %d\n", ec_capacity_ok(arg(2)), ec_limit_ok(arg(3)));
    } else if (argc == 7 && !strcmp(argv[1], "key")) {
        const uint32_t h = ec_hash(hex(2), hex(3), arg(4));
        printf("%u", h);
        for (int j = 0; j < AZ_EC_PROBE; ++j) printf(" %u", ec_bucket(h, j, (uint32_t)arg(5)));
        printf(" %d\n", ec_in_limit(hex(2), hex(3), arg(6)));
    } else if (argc == 5 && !strcmp(argv[1], "tag")) {
        const uint32_t stamp = ec_stamp((uint32_t)strtoul(argv[3], nullptr, 10), arg(4));
        const uint64_t tag = ec_tag((uint32_t)strtoul(argv[2], nullptr, 10), stamp);
        printf("%u %llx %u %u\n", stamp, (unsigned long long)tag, ec_tag_stamp(tag), ec_tag_hash(tag));
    } else if (argc == 3 && !strcmp(argv[1], "row")) {
        const int row = ec_row_of_entry(arg(2));
        printf("%d %d %d\n", row, ec_row_is_entry(row), ec_entry_of_row(row));
    } else if (argc == 3 && !strcmp(argv[1], "stride")) {
        printf("%d\n", ec_stride(arg(2)));
    } else if (argc == 6 && !strcmp(argv[1], "play")) {
        return play(arg(2), arg(3), arg(4), arg(5));
    } else {
        fprintf(stderr, "usage: %s rule REQUEST EVALUATOR GAME H W G BEYOND PROFILED | args CAPACITY LIMIT | key P1 M1 PLAYER CAPACITY LIMIT | tag HASH SERIAL SIM | row ENTRY | stride A | play CAPACITY LIMIT N SEED\n", argv[0]);
        return 2;
    }
    return 0;
}
