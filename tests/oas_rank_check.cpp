// Host build of the OtherAgentsStates rank (gym-exploration-2d_amd/csrc/cagym_oas_rank.h): tests/test_oas_rank_host.py compiles and runs this.
// Rows of keys are ranked in "waves" of 64 lanes, as the kernel does: every lane counts with oas_rank_fast; when ANY lane of the wave
// is not covered (oas_rank_covered) every lane of the wave takes oas_rank_exact.  Each result is held to the definition, written out
// here once more with nothing shared:  before(j) = #{ l : kl > kj  or  (kl == kj and l > j) }  over the live keys kj > -inf.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "cagym_oas_rank.h"

static const double NINF = -std::numeric_limits<double>::infinity();
static long long n_rows = 0, n_fast_lanes = 0, n_exact_lanes = 0, n_fast_waves = 0, n_exact_waves = 0, fails = 0;

static int definition(const double* k, int n, int j) {
    int before = 0;
    for (int l = 0; l < n; l++) {
        if (k[l] > k[j]) before++;
        else if (k[l] == k[j] && l > j) before++;
    }
    return before;
}

// one wave: lane i stands for key j[i] of row r[i] (N keys each)
template <int N>
static void wave(const std::vector<const double*>& rows, const std::vector<int>& js) {
    const int lanes = (int)rows.size();
    std::vector<OasRank> r(lanes);
    bool any = false;
    for (int i = 0; i < lanes; i++) {
        const double* k = rows[i];
        const double kj = k[js[i]];
        r[i] = oas_rank_fast<N>([&](int l) { return k[l]; }, kj);
        if (!oas_rank_covered(r[i], oas_key_bits(kj))) any = true;
    }
    (any ? n_exact_waves : n_fast_waves)++;
    for (int i = 0; i < lanes; i++) {
        const double* k = rows[i];
        const int j = js[i];
        const int got = (int)(any ? oas_rank_exact<N>([&](int l) { return k[l]; }, k[j], j) : r[i].gt);
        (any ? n_exact_lanes : n_fast_lanes)++;
        const int want = definition(k, N, j);
        // a covered lane's fast count is the definition's even when the wave falls back for another lane
        const bool covered = oas_rank_covered(r[i], oas_key_bits(k[j]));
        if (got != want || (covered && (int)r[i].gt != want)) {
            if (fails++ < 10) {
                printf("row of %d keys, key %d: got %d fast %d (covered %d) want %d :", N, j, got, (int)r[i].gt, (int)covered, want);
                for (int l = 0; l < N; l++) printf(" %a", k[l]);
                printf("\n");
            }
        }
    }
}

// all live keys of the rows in `pool` (N doubles each), 64 lanes at a time in row order - the kernel's dense index
template <int N>
static void rank_rows(const std::vector<double>& pool) {
    std::vector<const double*> rows;
    std::vector<int> js;
    const size_t nr = pool.size() / N;
    for (size_t r = 0; r < nr; r++) {
        n_rows++;
        for (int j = 0; j < N; j++) {
            if (!(pool[r * N + j] > NINF)) continue;
            rows.push_back(&pool[r * N]);
            js.push_back(j);
            if (rows.size() == 64) { wave<N>(rows, js); rows.clear(); js.clear(); }
        }
    }
    if (!rows.empty()) wave<N>(rows, js);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}
static double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }

template <int N>
static void random_rows(long long count, int special_every) {
    std::vector<double> pool((size_t)count * N);
    for (long long r = 0; r < count; r++) {
        double* k = &pool[(size_t)r * N];
        const int n = 1 + (int)(rnd() % N);  // live slots 0 .. n-1 but the own one
        const int own = (int)(rnd() % N);
        for (int l = 0; l < N; l++) k[l] = (l < n && l != own) ? 12.0 * uni() : NINF;
        if (special_every && r % special_every == 0) {
            const int what = (int)(rnd() % 6);
            for (int l = 0; l < n; l++) {
                if (l == own) continue;
                const uint64_t x = rnd();
                switch (what) {
                    case 0: if (x & 1) k[l] = -0.4 * uni(); break;                                  // overlapping agents
                    case 1: if (x & 1) k[l] = k[(int)((x >> 8) % n)] > NINF ? k[(int)((x >> 8) % n)] : k[l]; break;  // exact ties
                    case 2: if (x & 1) k[l] = (double)((x >> 8) % 3) * 4.9406564584124654e-324; break;   // +0 and subnormals, tied
                    case 3: if (x & 1) k[l] = -(double)(1 + (x >> 8) % 2) * 4.9406564584124654e-324; break;  // negative subnormals, tied
                    case 4: k[l] = (x & 1) ? -0.25 : ((x & 2) ? 0.25 : -0.5); break;               // ties among negatives and positives
                    case 5: if (x & 1) k[l] = ldexp(uni(), (int)((x >> 8) % 2000) - 1000) * ((x & 2) ? 1.0 : -1.0); break;  // every exponent
                }
            }
        }
    }
    rank_rows<N>(pool);
}

int main(int argc, char** argv) {
    const long long count = argc > 1 ? atoll(argv[1]) : 600000;
    // (1) every row of 4 keys over {-inf, a negative, +0, a positive, the positive again (a tie), the negative again}: 6^4 rows
    {
        const double vals[6] = {NINF, -0.375, 0.0, 1.5, 1.5, -0.375};
        std::vector<double> pool;
        for (int c = 0; c < 6 * 6 * 6 * 6; c++) {
            int x = c;
            for (int l = 0; l < 4; l++) { pool.push_back(vals[x % 6]); x /= 6; }
        }
        // each row alone in its wave (the path depends on that row only), then all of them packed
        for (size_t r = 0; r < pool.size() / 4; r++) rank_rows<4>(std::vector<double>(pool.begin() + r * 4, pool.begin() + r * 4 + 4));
        rank_rows<4>(pool);
    }
    // (2) random rows of 10 and 20 keys; every `special_every`-th row has ties, negative keys, subnormals: with 1 in 40 about one
    // wave in five falls back, with 1 in 2 nearly every one
    random_rows<10>(count, 40);
    random_rows<10>(count / 4, 2);
    random_rows<20>(count, 40);
    random_rows<20>(count / 4, 2);
    random_rows<10>(count / 4, 0);
    printf("rows %lld fast waves %lld exact waves %lld fast lanes %lld exact lanes %lld fails %lld\n", n_rows, n_fast_waves, n_exact_waves,
           n_fast_lanes, n_exact_lanes, fails);
    if (!fails && n_fast_waves > 1000 && n_exact_waves > 1000) printf("oas_rank_check ok\n");
    return fails ? 1 : 0;
}
