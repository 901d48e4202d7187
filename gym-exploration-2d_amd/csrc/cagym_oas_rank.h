// cagym_oas_rank.h -- the row of one other agent in the OtherAgentsStates table: how many keys of the ego's key row sort before it.
//
// The order is OtherAgentsStatesSensor's (sensors/OtherAgentsStatesSensor.py:28-34, a stable ascending sort, reversed): descending
// key, ties by descending slot.  Key l is before key j exactly when
//         (kl > kj) || (kl == kj && l > j)                                                      (the definition: oas_before_exact)
// The fast path counts with the keys' BITS as signed 64-bit integers, one compare and one add-with-carry per key, and a second
// compare and add that counts the keys whose bits equal kj's:
//   * a key kj >= +0 has the sign bit clear; among such doubles the signed order of the bits is the order of the values, and every
//     key with the sign bit set (-inf: own slot, padding, absent agents; a negative key: overlapping agents) is a negative integer,
//     below kj as an integer and below it as a double.  So for kj >= +0:  kl > kj  <=>  bits(kl) > bits(kj),  and -inf stays
//     "never before".
//   * with no second key of the same bits (the count of equal bits is 1: kj itself) the tie rule never applies.
// A lane whose kj has the sign bit set (negative keys order backwards as integers) or whose count of equal bits is not 1 is not
// covered: the caller then runs the definition for every lane of the wave (oas_rank_covered / oas_rank_exact), so the result is
// the definition's on every input the fast path is used for.
// Inputs the pair phase cannot produce, and which the two paths would treat differently: NaN (its bits order as a large number;
// positions and radii are finite) and -0 (equal to +0 as a double, not as bits).  A key is (d - r_a) - r_b with d = sqrt(..) >= +0,
// and x - y is -0 only for (-0) - (+0): neither difference can be -0.
// A form the host compiler accepts (tests/test_oas_rank_host.py compiles tests/oas_rank_check.cpp against it), as cagym_spin.h.
#pragma once

#ifndef CAGYM_RANK_HD
#ifdef __HIPCC__
#define CAGYM_RANK_HD __host__ __device__ __forceinline__
#else
#define CAGYM_RANK_HD inline
#endif
#endif

CAGYM_RANK_HD long long oas_key_bits(double k) {
    long long b;
    __builtin_memcpy(&b, &k, sizeof b);
    return b;
}

struct OasRank {  // (unsigned: sums the compiler may not widen to the 64 bits of the row's address)
    unsigned gt;  // keys whose bits are above kj's as signed integers
    unsigned eq;  // keys of the same bits (kj itself among them)
};

CAGYM_RANK_HD void oas_rank_add(OasRank& r, double kl, long long bj) {
    const long long bl = oas_key_bits(kl);
    r.gt += bl > bj ? 1u : 0u;
    r.eq += bl == bj ? 1u : 0u;
}
// r.gt is the definition's count
CAGYM_RANK_HD bool oas_rank_covered(const OasRank& r, long long bj) { return bj >= 0 && r.eq == 1u; }

CAGYM_RANK_HD unsigned oas_before_exact(double kl, double kj, int l, int j) { return ((kl > kj) || (kl == kj && l > j)) ? 1u : 0u; }

// the two counts over a row of N keys held by `key(l)` (registers: N is a compile-time bound, the loops unroll)
template <int N, typename Keys>
CAGYM_RANK_HD OasRank oas_rank_fast(Keys key, double kj) {
    const long long bj = oas_key_bits(kj);
    OasRank r = {0, 0};
#pragma unroll
    for (int l = 0; l < N; l++) oas_rank_add(r, key(l), bj);
    return r;
}
template <int N, typename Keys>
CAGYM_RANK_HD unsigned oas_rank_exact(Keys key, double kj, int j) {
    unsigned before = 0;
#pragma unroll
    for (int l = 0; l < N; l++) before += oas_before_exact(key(l), kj, l, j);
    return before;
}
