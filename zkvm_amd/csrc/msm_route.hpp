// msm_route.hpp -- which form of the multiscalar multiplication a call takes, and the bytes of every workspace buffer that form
// writes: the per-point tables or the bucket pipeline, the window width, the partition sort or count / scan / scatter, the
// reduce form, the chunking of a window.  Settled from the sizes of the call alone, before its first launch.
// No HIP here: run_to_windows and the batch entry points (zkgpu.hip) and the CPU tests (libzkhost, zkhost_msm_route) run the
// same function.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace zk {

// what zkgpu.hip holds against kernels.hpp (static_assert there): words per point, buckets per reduce task, the tiles of the
// scan and of the partition sort, the bin classes
constexpr int ROUTE_EXT_WORDS = 40, ROUTE_NIELS_WORDS = 32, ROUTE_DEC_WORDS = 64;
constexpr int ROUTE_REDUCE_CHUNK = 64;
#ifdef ZK_REDUCE_CHUNK_BIG
constexpr int ROUTE_REDUCE_CHUNK_BIG = ZK_REDUCE_CHUNK_BIG;
#else
constexpr int ROUTE_REDUCE_CHUNK_BIG = 16;
#endif
constexpr int ROUTE_SCAN_TILE = 2048, ROUTE_PART_TILE = 2048, ROUTE_PART_LO_BITS = 8, ROUTE_PART_IDX_BITS = 23, ROUTE_SIZE_CLASSES = 256;
constexpr uint32_t ROUTE_FAT_BIN = 96, ROUTE_HEAVY_MAX = 65536;
constexpr int ROUTE_FAT_LANES = 16;

constexpr uint64_t PART_SORT_MIN_TERMS = 32768;     // terms from which a single multiplication is sorted by partitions
constexpr uint64_t QUAD_REDUCE_MAX_TASKS = 65536;   // reduce tasks up to which a quad of lanes takes each
constexpr uint64_t SPLIT_DECODE_MIN_POINTS = 131072; // points from which the decoder's squaring chain is a kernel of its own
constexpr uint64_t SMALL_MIN_ROWS = 64, SMALL_MAX_ROW = 256, SMALL_TERMS_PER_ROW = 64, SMALL_TERMS_PER_ROW_TABLES = 128;

// wavefronts per MSM in k_small_accumulate: about three per SIMD (1024 SIMDs) over the whole launch
inline int small_parts(uint64_t B) {
  return (int)std::max<uint64_t>(1, std::min<uint64_t>(4, (3072 + B / 2) / std::max<uint64_t>(B, 1)));
}

// window width minimising  W * (terms + 2 * 2^(w-1) * msms)  point additions
inline int choose_window(uint64_t n_terms, uint32_t n_msm) {
  double per = (double)n_terms / (n_msm ? n_msm : 1);
  int best = 4; double best_cost = 1e300;
  for (int w = 4; w <= 16; ++w) {
    double W = 255 / w + 1;
    double reduce = 2.0 * (double)(1u << (w - 1));
    if ((1u << (w - 1)) > (unsigned)ROUTE_REDUCE_CHUNK) reduce *= 1.3;  // chunk fix-up work
    double cost = W * (per + reduce);
    if (cost < best_cost) { best_cost = cost; best = w; }
  }
  return best;
}

// who asks: a call that goes to the bucket pipeline whatever its shape (the single multiplication; a batch that has been
// routed already), zkgpu_msm_batch / zkgpu_verify_batch*, or the proof-specific half of a batch over a point set with tables
enum { MSM_DIRECT = 0, MSM_BATCH = 1, MSM_TABLES = 2 };

// rows, proof-specific terms, generator terms (MSM_TABLES: summed out of the tables, no part of the route), the longest row of
// proof-specific terms (~0: not known), a forced window width (0: none)
struct MsmShape { uint64_t n_msm, n_dyn, n_static, max_dyn_row; int forced_w, entry; };

struct MsmRoute {
  bool small; int parts;             // per-point tables and one workgroup of `parts` wavefronts per row | the bucket pipeline
  int w, n_windows;                  // small: 4, 64
  // the bucket pipeline (all zero when small)
  uint32_t n_buckets, chunk_size, chunks;
  uint64_t n_terms, n_wins, n_bins, n_tasks, max_entries;
  bool too_large;                    // past 32-bit entry indices: the call is refused
  bool part_sort, quad_reduce, window_partials, split_decode;
  uint32_t scan_blocks, fat_cap, fat_blocks;
  uint32_t hi_bits, n_part, n_tiles; // the partition sort's shape (part_sort only)
  // bytes per workspace buffer
  size_t dyn_rows, bins, block_sums, entries, buckets, partials, partial_flags, window_sums, window_flags, msm_fail, heavy, class_count,
      bin_order, dec_scratch, part_hist, part_block_sums, part_entries;
};

inline MsmRoute plan_msm(const MsmShape& sh) {
  MsmRoute r = {};
  const uint64_t B = sh.n_msm;
  // many SMALL multiplications: EVERY row must be short, not just the average, and the caller must be able to see the rows
  if (sh.entry == MSM_BATCH)
    r.small = !sh.forced_w && sh.n_static == 0 && sh.n_dyn && sh.n_dyn <= SMALL_TERMS_PER_ROW * B && B >= SMALL_MIN_ROWS && sh.max_dyn_row <= SMALL_MAX_ROW;
  else if (sh.entry == MSM_TABLES)
    r.small = !sh.forced_w && sh.n_dyn <= SMALL_TERMS_PER_ROW_TABLES * B;
  if (r.small) {
    r.parts = small_parts(B);
    r.w = 4; r.n_windows = 64;
    return r;
  }
  const uint64_t n_static = sh.entry == MSM_TABLES ? 0 : sh.n_static;
  r.n_terms = sh.n_dyn + n_static;
  r.w = std::max(2, std::min(16, sh.forced_w ? sh.forced_w : choose_window(r.n_terms, (uint32_t)B)));
  r.n_windows = 255 / r.w + 1;
  r.n_buckets = 1u << (r.w - 1);
  r.n_wins = B * r.n_windows;
  r.n_bins = r.n_wins * r.n_buckets;
  r.chunk_size = r.n_buckets <= (uint32_t)ROUTE_REDUCE_CHUNK ? r.n_buckets : (uint32_t)ROUTE_REDUCE_CHUNK_BIG;
  r.chunks = (r.n_buckets + r.chunk_size - 1) / r.chunk_size;
  r.n_tasks = r.n_wins * r.chunks;
  r.max_entries = r.n_terms * r.n_windows;
  r.too_large = r.max_entries >= (1ull << 32) || r.n_bins >= (1ull << 32) || sh.n_dyn >= (1ull << 30) || n_static >= (1ull << 32);
  if (r.too_large) return r;
  r.scan_blocks = (uint32_t)((r.n_bins + ROUTE_SCAN_TILE - 1) / ROUTE_SCAN_TILE);
  // single large multiplication: two-level sort with LDS atomics only (its entries carry a 23-bit term index)
  r.part_sort = B == 1 && n_static == 0 && r.w - 1 >= ROUTE_PART_LO_BITS && r.n_terms >= PART_SORT_MIN_TERMS && r.n_terms <= (1ull << ROUTE_PART_IDX_BITS);
  // few tasks (one large multiplication: 32 768): a quad of lanes per task, a third of the chain's depth; many tasks (a batch
  // of small ones): one lane each, a quarter of the instructions
  r.quad_reduce = r.n_tasks <= QUAD_REDUCE_MAX_TASKS;
  r.window_partials = r.chunks > 1;
  r.split_decode = sh.n_dyn >= SPLIT_DECODE_MIN_POINTS;
  r.fat_cap = (uint32_t)(r.max_entries / ROUTE_FAT_BIN + 64);
  r.fat_blocks = std::min<uint32_t>((uint32_t)(((uint64_t)r.fat_cap * ROUTE_FAT_LANES + 255) / 256), 320u);
  const size_t ext = (size_t)ROUTE_EXT_WORDS * 4;
  r.dyn_rows = (size_t)(std::max<uint64_t>(sh.n_dyn, 1) * ROUTE_NIELS_WORDS * 4);
  r.bins = (size_t)((r.n_bins + 1) * 4);
  r.block_sums = ((size_t)r.scan_blocks + 1) * 4;
  r.entries = (size_t)(std::max<uint64_t>(r.max_entries, 1) * 4);
  r.buckets = (size_t)(r.n_bins * ext);
  r.partials = (size_t)(r.n_tasks * ext);
  r.partial_flags = (size_t)(r.n_tasks * 4);
  r.window_sums = (size_t)(r.n_wins * ext);
  r.window_flags = (size_t)(r.n_wins * 4);
  r.msm_fail = (size_t)B * 4;
  r.heavy = ((size_t)ROUTE_HEAVY_MAX + 1 + r.fat_cap + 1) * 4;       // heavy list | fat list, each behind its count
  r.class_count = (size_t)2 * ROUTE_SIZE_CLASSES * 4;
  r.bin_order = (size_t)(r.n_bins * 4);
  r.dec_scratch = r.split_decode ? (size_t)(sh.n_dyn * ROUTE_DEC_WORDS * 4) : 0;
  if (r.part_sort) {
    r.hi_bits = (uint32_t)(r.w - 1 - ROUTE_PART_LO_BITS);
    r.n_part = (uint32_t)r.n_windows << r.hi_bits;
    r.n_tiles = (uint32_t)((r.n_terms + ROUTE_PART_TILE - 1) / ROUTE_PART_TILE);
    r.part_hist = (size_t)((uint64_t)r.n_part * r.n_tiles * 4);
    r.part_block_sums = ((size_t)2 * r.n_part + 4) * 4;              // block_sums again: totals[n_part] | part_base[n_part + 1] | ticket
    r.part_entries = r.entries;
  }
  return r;
}

}  // namespace zk
