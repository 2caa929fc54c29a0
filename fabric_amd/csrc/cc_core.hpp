// Connected-component labelling: the integer helpers of cc.hip that have no GPU-specific arithmetic -- run seeding, the choice of the
// links between two neighbouring rows, find and the decreasing-parent union -- as plain functions, so that a stand-alone host program
// (tools/cc_host_check.cpp, built with -fsanitize=address,undefined) can run them serially over the test patterns before a kernel runs.
// The parent array is reached through a policy P: int load(int i) and int fetch_min(int i, int v) (returns the old value).  cc.hip gives
// LDS and global-memory policies whose fetch_min is an atomicMin; the host program a serial one.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CC_HD __host__ __device__ __forceinline__
#else
#define CC_HD inline
#endif

constexpr int CC_TILE = 64;                               // tile edge: one 64-bit mask per tile row

// Column of the first pixel of the run of set bits of m that holds column c (bit c of m is set).
CC_HD int cc_run_start(uint64_t m, int c) {
    const uint64_t z = ~m & ((1ull << c) - 1);            // the clear bits below c
    return z ? 64 - __builtin_clzll(z) : 0;
}

// Links of the foreground pixel at column c of a row with mask m to the neighbouring row with mask mu (the row above, or across a seam):
// bit 0 = column c - 1, bit 1 = c, bit 2 = c + 1 of mu.  Only the links that no other column of the same pair of runs makes:
//   the pixel above is set: it alone (c - 1 and c + 1 above then belong to its run), and not even it when column c - 1 holds the same
//     pair (set in both rows) -- the first column of an overlap makes the link;
//   otherwise, 8-connectivity only: the diagonal c - 1 when this row's run starts at c (a set m[c - 1] has that pixel straight above it),
//     and the diagonal c + 1 when this row's run ends at c.
// nbits: the width of both masks (bits at and above it are clear).
CC_HD int cc_links(uint64_t m, uint64_t mu, int c, int nbits, int connectivity) {
    if (!(m >> c & 1)) return 0;
    const bool hl = c > 0, hr = c + 1 < nbits;
    const bool L = hl && (m >> (c - 1) & 1), R = hr && (m >> (c + 1) & 1);
    const bool uL = hl && (mu >> (c - 1) & 1), uC = mu >> c & 1, uR = hr && (mu >> (c + 1) & 1);
    if (uC) return L && uL ? 0 : 2;
    if (connectivity != 8) return 0;
    return (uL && !L ? 1 : 0) | (uR && !R ? 4 : 0);
}

// Follows parents from a.  parent[i] <= i always, so `a` strictly decreases until parent[a] == a: at most a + 1 <= cap steps.  The value
// is a hint only (a stale read gives an older ancestor of the same set): no decision hangs on it.  *status is raised if the cap is hit.
template <class P> CC_HD int cc_find(P& par, int a, int cap, int* status) {
    for (int it = 0; it <= cap; it++) {
        const int p = par.load(a);
        if (p == a) return a;
        a = p;
    }
    *status = 1;
    return a;
}

// The decreasing-parent union.  Every decision comes from fetch_min's return value.  Each pass replaces the pair (a, b), a > b, by
// (old, b) with old < a: max(a, b) strictly decreases, so there are at most max(a, b) + 1 <= cap passes.  A parent only ever gets a
// smaller member of its own set, and a root r keeps parent[r] == r until a smaller member is hung under it, so the last root of a set is
// its smallest index whatever the order of the unions.
template <class P> CC_HD void cc_union(P& par, int a, int b, int cap, int* status) {
    a = cc_find(par, a, cap, status);
    b = cc_find(par, b, cap, status);
    for (int it = 0; a != b; it++) {
        if (it > cap) { *status = 1; return; }
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = par.fetch_min(a, b);
        if (old == a) return;                              // a was a root and now hangs under b
        a = old;                                           // a had a parent: the sets of old and b are still to be joined
    }
}
