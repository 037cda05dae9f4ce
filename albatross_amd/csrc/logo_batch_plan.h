// logo_batch_plan.h — the pooled plan of agp_logo_nll_gradient_batch: the non-empty groups of ALL problems of a call sorted
// by (size, problem, group) and cut into chunks that advance in lock step, so the number of launch chains follows the size
// classes of the whole batch, not the number of problems or groups.  Plain C++ (no HIP, no context): gradient.hip runs it,
// agp_debug_logo_batch_plan (debug_api.hip) shows it to tests/test_logo_gradient_batch_host.py without a device, and
// examples/host_sanitize_check.cpp walks it under the sanitizers.  logo_plan (gradient.hip) stays the plan of one problem.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace agp {

// the limits of one chunk (those of logo_plan): the largest group at most 2x the smallest, at most groups_max groups,
// img_elems_max doubles of tile images, cols_max padded columns (what the carve provides: count * n of the call)
struct LogoBatchLimits {
  long long groups_max, img_elems_max, cols_max;
  long long (*ld_of)(long long);          // leading dimension of an m x m block slab (factor_ld)
  long long (*img_stride_of)(long long);  // doubles of one block's tile images (logo_img_stride)
};

// `count` groups padded to m.  In LogoBatchPlan::meta: idx_off, count * m point indices (row numbers inside the group's own
// problem, -1 = padding); size_off, count real sizes; prob_off, count problems.  term_off: the chunk's first term.
struct LogoBatchChunk {
  long long m, count, idx_off, size_off, prob_off, term_off;
};

struct LogoBatchPlan {
  std::vector<long long> meta;  // the chunk tables, then csr_off (problems + 1 words at csr_at) and csr_terms (terms words)
  std::vector<LogoBatchChunk> chunks;
  std::vector<long long> problem, group, size;  // term q: group group[q] (the caller's number) of problem problem[q]
  long long terms = 0, problems = 0;
  long long csr_at = 0, csr_terms_at = 0;  // problem b's terms: meta[csr_terms_at + meta[csr_at + b] .. + meta[csr_at + b + 1])
  size_t block_elems = 0, img_elems = 0, vec_elems = 0, count_elems = 0;  // the largest chunk's slab, images, vectors, scalars
};

// false for malformed offsets, an index outside [0, n_b), or an index that occurs twice in its problem; empty groups are
// dropped, points in no group are allowed, a problem may have no group at all.
inline bool logo_batch_plan(long long count, const long long *n, const int64_t *n_groups, const int64_t *const *offsets,
                            const int64_t *const *indices, const LogoBatchLimits &lim, LogoBatchPlan &p) {
  if (count <= 0 || !n || !n_groups) return false;
  struct Item { long long m, b, g; };
  std::vector<Item> order;
  std::vector<char> seen;
  for (long long b = 0; b < count; ++b) {
    const long long ng = n_groups[b];
    if (n[b] <= 0 || ng < 0) return false;
    if (ng == 0) continue;
    const int64_t *off = offsets ? offsets[b] : nullptr;
    if (!off || off[0] != 0) return false;
    for (long long g = 0; g < ng; ++g) {
      const long long m = off[g + 1] - off[g];
      if (m < 0) return false;
      if (m > 0) order.push_back(Item{m, b, g});
    }
    const long long total = off[ng];
    if (total > n[b]) return false;  // (more than n_b indices: one occurs twice)
    const int64_t *ind = indices ? indices[b] : nullptr;
    if (total > 0 && !ind) return false;
    seen.assign((size_t)n[b], 0);
    for (long long i = 0; i < total; ++i) {
      const long long j = ind[i];
      if (j < 0 || j >= n[b] || seen[(size_t)j]) return false;
      seen[(size_t)j] = 1;
    }
  }
  std::sort(order.begin(), order.end(), [](const Item &x, const Item &y) {
    return x.m != y.m ? x.m < y.m : (x.b != y.b ? x.b < y.b : x.g < y.g);
  });
  p.problems = count;
  p.terms = (long long)order.size();
  for (const Item &o : order) { p.problem.push_back(o.b); p.group.push_back(o.g); p.size.push_back(o.m); }
  size_t at = 0;
  while (at < order.size()) {
    const long long m0 = order[at].m;
    size_t end = at + 1;
    while (end < order.size()) {
      const long long m = order[end].m, cnt = (long long)(end - at) + 1;
      if (m > 2 * m0 || cnt > lim.groups_max || cnt * m > lim.cols_max || cnt * lim.img_stride_of(m) > lim.img_elems_max) break;
      ++end;
    }
    LogoBatchChunk ch;
    ch.m = order[end - 1].m;
    ch.count = (long long)(end - at);
    ch.term_off = (long long)at;
    ch.idx_off = (long long)p.meta.size();
    p.meta.resize(p.meta.size() + (size_t)(ch.count * ch.m), -1);
    for (size_t q = at; q < end; ++q) {
      const Item &o = order[q];
      const int64_t *src = indices[o.b] + offsets[o.b][o.g];
      for (long long a = 0; a < o.m; ++a) p.meta[(size_t)ch.idx_off + (size_t)((long long)(q - at) * ch.m + a)] = src[a];
    }
    ch.size_off = (long long)p.meta.size();
    for (size_t q = at; q < end; ++q) p.meta.push_back(order[q].m);
    ch.prob_off = (long long)p.meta.size();
    for (size_t q = at; q < end; ++q) p.meta.push_back(order[q].b);
    p.chunks.push_back(ch);
    const size_t blocks = (size_t)ch.count * (size_t)(lim.ld_of(ch.m) * ch.m), imgs = (size_t)ch.count * (size_t)lim.img_stride_of(ch.m);
    const size_t vec = (size_t)((ch.count * ch.m + 1) / 2 * 2), cnt2 = (size_t)((ch.count + 1) / 2 * 2);
    p.block_elems = std::max(p.block_elems, blocks);
    p.img_elems = std::max(p.img_elems, imgs);
    p.vec_elems = std::max(p.vec_elems, vec);
    p.count_elems = std::max(p.count_elems, cnt2);
    at = end;
  }
  // the terms of every problem in ascending term order (the order of its fixed-order sum), in CSR form
  p.csr_at = (long long)p.meta.size();
  p.meta.resize(p.meta.size() + (size_t)count + 1, 0);
  for (long long q = 0; q < p.terms; ++q) ++p.meta[(size_t)p.csr_at + (size_t)p.problem[(size_t)q] + 1];
  for (long long b = 0; b < count; ++b) p.meta[(size_t)p.csr_at + (size_t)b + 1] += p.meta[(size_t)p.csr_at + (size_t)b];
  p.csr_terms_at = (long long)p.meta.size();
  p.meta.resize(p.meta.size() + (size_t)p.terms, 0);
  std::vector<long long> fill((size_t)count, 0);
  for (long long q = 0; q < p.terms; ++q) {
    const size_t b = (size_t)p.problem[(size_t)q];
    p.meta[(size_t)p.csr_terms_at + (size_t)(p.meta[(size_t)p.csr_at + b] + fill[b]++)] = q;
  }
  return true;
}

}  // namespace agp
