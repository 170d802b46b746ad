// Which (block, head, batch) a workgroup of the v2 attention kernels takes,
// as a function of its linear block id.  Plain integers and no HIP types, so
// a host program can include this header and check the map exhaustively
// (tests/ops/test_attn_work_order_cpu.py).
//
// Two facts about the hardware shape the map: workgroups are dispatched in
// increasing linear id L = x + nx*(y + gy*z), and id L runs on XCD L % 8 (each
// XCD has its own L2).  Under a causal or shifted-causal mask the work of a
// block is monotone in its index along S: a late q block loops over more kv
// tiles, an early kv block over more q tiles.  The map therefore
//
//   * keeps all nx blocks of one group (a (head, batch) pair, G = gy*gz of
//     them) on one XCD when G % 8 == 0, so the group's K/V (or Q/dO) stay in
//     that XCD's L2 and every XCD gets the same multiset of block weights;
//   * hands out ranks in increasing order within an XCD, rank 0 being the
//     heaviest block, so the long workgroups start first and the short ones
//     fill the tail (longest-processing-time-first list scheduling).
//
// When G % 8 != 0 no XCD pinning is possible with a static map and the order
// is plain heaviest-first: rank = L / G, group = L % G.
//
// The caller turns the rank into its block index: nx-1-rank where late blocks
// are heavy (forward, dq), rank where early blocks are heavy (dkdv).  A fully
// visible launch has equal weights and is indifferent to the order.  The map
// is a bijection of [0, nx*gy*gz) onto nx x gy x gz for every grid, so it
// changes which workgroup computes a tile and when, never what is computed.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ATTN_WORK_ORDER_HD __host__ __device__
#else
#define ATTN_WORK_ORDER_HD
#endif

struct AttnWork {
    int rank;  // 0 = heaviest block of its group, nx-1 = lightest
    int h;     // grid y: head (the KV head for dkdv)
    int b;     // grid z: batch
};

constexpr unsigned ATTN_NUM_XCD = 8;

// L in [0, nx*gy*gz); nx itself is not needed: rank = L / (gy*gz) up to the
// XCD interleave, so rank < nx follows from the range of L.
ATTN_WORK_ORDER_HD inline AttnWork attn_work_order(unsigned L, unsigned gy,
                                                   unsigned gz) {
    const unsigned G = gy * gz;
    unsigned rank, group;
    if (G % ATTN_NUM_XCD == 0) {
        const unsigned per_xcd = G / ATTN_NUM_XCD;  // groups on one XCD
        const unsigned xcd = L % ATTN_NUM_XCD;
        const unsigned slot = L / ATTN_NUM_XCD;     // position in the XCD's queue
        rank = slot / per_xcd;
        group = ATTN_NUM_XCD * (slot % per_xcd) + xcd;
    } else {
        rank = L / G;
        group = L % G;
    }
    return AttnWork{(int)rank, (int)(group % gy), (int)(group / gy)};
}
