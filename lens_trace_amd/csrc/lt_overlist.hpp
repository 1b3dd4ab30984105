// lt_overlist.hpp -- overlap lists (lt_overlist.hip; lt_hip_overlap_boxes_list and lt_hip_overlap_tris_list in lt_capi.hip): every
// primitive a box or a query triangle touches, as CSR -- offsets[n + 1] in uint64, items[offsets[n]] in int32.  The call is
//   count   the box or triangle walk with lt_overlap::kCountWide: the sequence's length of query i, as uint64, into offsets[i];
//   scan    an exclusive scan in place over the n + 1 words (word n counts as 0 on the way in and holds the total after);
//   fill    the same walk with lt_overlap::kList: query i's touching offsets into its segment, in walk order;
//   order   each segment sorted ascending, so that the words are the sequence of include/lenstrace_hip.h -- a function of the scene
//           and the query alone, whichever hierarchy was walked.  (The words are offsets only, so the sorted multiset is the
//           sequence: its second key, the node index, orders equal words.)
// No kernel waits for another workgroup: the scan is three launches, and a segment is sorted by the one wave that took it.
// The radius lists (lt_hip_nearest_list) are the same four steps with lt_nearest.hip's walk and its kinds of the same names; their
// items are 16-byte records {d2, prim, u, v}, ordered by (d2, prim).
// The hit lists (lt_hip_trace_hits_list) are the four steps once more with lt_query.hip's walks: 16-byte records {t, prim, u, v},
// ordered by t and, among bit-equal t, by the reference's traversal order -- for the rays the own tree takes through the scene's
// rank table in the ordering kernel, for the others by a stable insertion during the fill.
#pragma once
#include <stdint.h>

namespace lt_overlist {

// Words of offsets per workgroup of the scan's first and third launch (256 lanes, eight words each).
constexpr uint32_t kListScanTile = 2048;
// The longest segment that is sorted in LDS: 16 KB per wave.  Longer ones are sorted in place in global memory.
constexpr uint32_t kListSortSpan = 4096;
// The same for 16-byte records (lt_hip_nearest_list, lt_hip_trace_hits_list): 16 KB per wave again, ten waves per CU.
constexpr uint32_t kListSortSpanHits = 1024;

// Partial sums the scan of n queries needs (one uint64 per tile of the n + 1 words).
inline uint64_t scan_partials(uint64_t n) { return (n + 1 + kListScanTile - 1) / kListScanTile; }

constexpr uint32_t kScanLaunches = 3, kOrderLaunches = 1;

}  // namespace lt_overlist

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>

namespace lt_overlist {

// The exclusive scan in place over offsets[0 .. n]: offsets[i] becomes the sum of the words before it, offsets[n] the total.
// `partials`: scan_partials(n) words of scratch.  Three launches on `s`.
hipError_t scan(unsigned long long* offsets, uint32_t n, unsigned long long* partials, hipStream_t s);

// Sorts items[offsets[i] .. min(offsets[i + 1], capacity)) ascending for every i < n (a negative length is 0).  oneShot: the
// offsets are this stream's own scan, and when offsets[n] > capacity nothing is touched.  One launch on `s`.
hipError_t order(const unsigned long long* offsets, uint32_t n, int32_t* items, unsigned long long capacity, bool oneShot, uint32_t cuCount,
                 hipStream_t s);

// The same over 16-byte records {d2, prim, u, v}, ascending by lt_nearest::record_before -- (d2, prim); records that are equal in
// both are bit-identical, so the order among them is no one's to see.  One launch on `s`.
hipError_t order_hits(const unsigned long long* offsets, uint32_t n, uint4* items, unsigned long long capacity, bool oneShot, uint32_t cuCount,
                      hipStream_t s);

// The same over a hit list's records {t, prim, u, v}, for the rays the own tree takes (lt_query::own_tree_takes on rays[i]; the
// other rays' segments are sorted already and stay untouched): ascending t by the float `<`, bit-equal t by rank8[8 prim + octant],
// the octant ray i's (nPrims: the table's rows).  rank8 null -- a scene without an own tree -- launches nothing.  One launch on `s`, or none.
hipError_t order_ray_hits(const unsigned long long* offsets, uint32_t n, uint4* items, unsigned long long capacity, bool oneShot,
                          const float4* rays, const uint32_t* rank8, uint32_t nPrims, uint32_t cuCount, hipStream_t s);

}  // namespace lt_overlist
#endif
