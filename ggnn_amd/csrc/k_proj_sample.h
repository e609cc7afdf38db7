// k_proj_sample.h -- projective dependency trees drawn on the device from the
// distribution whose arc marginals k_marg.h computes: the weight of a tree is
// the product of its words' head probabilities, over the trees without
// crossing arcs (ROOT leftmost).  One inside pass (k_marg.h's marg_inside: the
// same tables, potentials and ln Z) serves every sample of a graph; a sample is
// a top-down walk over the tables of at most 2 m - 1 draws.  Host form:
// evaluation.py projective_sample_arrays.
//
// An item (kind, s, t) stands for one table entry (positions and packing are
// k_marg.h's) and is expanded by one draw over its terms, in ascending r:
//   0  ROOT's child (single_root)  r = 0..m-1  CL[0][r] + CR[r][m-1] + psi(r+1 takes ROOT)
//   1  CR[s][t], s < t             r = s+1..t  IR[s][r] + CR[r][t]
//   2  CL[s][t], s < t             r = s..t-1  CL[s][r] + IL[r][t]
//   3  IR[s][t]                    r = s..t-1  CR[s][r] + CL[r+1][t]    node lo+t takes lo+s
//   4  IL[s][t]                    as kind 3                            node lo+s takes lo+t
// The two entries of the chosen term are the item's children; a complete span
// with s = t is a leaf.  The start item is kind 0, CR[0][m-1] without
// single_root.  The order in which pending items are expanded does not matter:
//   masses   q_r = expf(term_r - M), M the largest term, 0 for a -inf term (the
//            per-word constants of the potentials cancel inside an item);
//   draw     u = (x >> 8) * 2^-24, x the first word of Philox4x32-10 at counter
//            (kind << 16 | s << 8 | t, sample, graph, 0x50000000) under the
//            64-bit seed.  With inclusive prefix sums c_r in ascending r and S
//            the last: the smallest r with q_r > 0 and c_r > u S, the largest r
//            with q_r > 0 if rounding leaves none (k_tree_sample.h's rule).
// A chosen term is finite, so both children have a derivation: a returned
// sample is a projective tree over allowed arcs with the right ROOT count by
// construction.  S not > 0 is the only dead end (status 2).
//
// Every projective tree has one derivation: an arc adds one I item and every
// expanded C item has one I child, so a sample expands at most 2 (m - 1) + 1
// items.  The pending items are a frontier of that derivation: their spans lie
// side by side in 0..m-1 and each has s < t, so at most m - 1 <= TREE_MAXV - 1
// are pending at once: the stack of PROJ_SAMPLE_STACK entries cannot overflow
// (a push that would is a dead end all the same).
//
// One workgroup of 256 threads per (graph, chunk of PROJ_SAMPLE_CHUNK
// consecutive samples).  The workgroup fills the tables as
// k_projective_marginals does; then wave w walks the chunk's samples w, w + 4,
// ... on its own: the tables are read-only by then, the stack and the sample's
// heads lie in the wave's own LDS rows, and every lane writes the same values
// there, so no barrier is needed.  One item per step: lane l holds the terms l,
// l + 64, ... (one segment for an item of up to 64 terms, four above), the
// maximum by butterfly, the prefix sums by a shuffle scan per segment with the
// segments' totals added in order, the choice by ballot.  No atomics, nothing
// between workgroups, every scan and reduction in a fixed order: sample s of
// graph g depends on (seed, g, s) alone and two launches give the same bytes.
#pragma once
#include <cfloat>

#include "k_marg.h"

#define PROJ_SAMPLE_LDS_MAXN 128  // GGNN_PROJ_SAMPLE_LDS_MAXN
#define PROJ_SAMPLE_CHUNK 16      // GGNN_PROJ_SAMPLE_CHUNK
#define PROJ_SAMPLE_STACK TREE_MAXV
#define PROJ_SAMPLE_STREAM 0x50000000u
#define PROJ_SAMPLE_LDS_BYTES \
  (sizeof(float) * (4 * PROJ_TRI(PROJ_SAMPLE_LDS_MAXN) + TREE_MAXV + 2) + sizeof(int) * 4 * (PROJ_SAMPLE_STACK + TREE_MAXV))

static_assert(TREE_MAXV <= 256, "an item packs s and t into a byte each");
static_assert(PROJ_SAMPLE_STACK >= TREE_MAXV - 1, "at most m - 1 items are pending");
static_assert(PROJ_SAMPLE_LDS_BYTES <= 160 * 1024, "tables, c[], four stacks and head rows fit the LDS of a CU");

// One draw by a whole wave: q[t] is the mass of term lane + 64 t.  Returns the
// drawn term, -1 when the masses do not sum to > 0; the same in every lane.
template <int NS>
DEV int proj_sample_pick(const float (&q)[NS], float u, int lane) {
  float run[NS], c[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) run[t] = q[t];
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) {
#pragma unroll
    for (int t = 0; t < NS; ++t) {
      const float up = __shfl_up(run[t], w);
      if (lane >= w) run[t] += up;
    }
  }
  float total = 0.f;
#pragma unroll
  for (int t = 0; t < NS; ++t) {
    c[t] = total + run[t];
    total += __shfl(run[t], 63);
  }
  if (!(total > 0.f)) return -1;
  const float target = u * total;
#pragma unroll
  for (int t = 0; t < NS; ++t) {
    const unsigned long long hit = __ballot(q[t] > 0.f && c[t] > target);
    if (hit) return 64 * t + __ffsll(hit) - 1;
  }
#pragma unroll
  for (int t = NS - 1; t >= 0; --t) {
    const unsigned long long live = __ballot(q[t] > 0.f);
    if (live) return 64 * t + 63 - __clzll(live);
  }
  return -1;
}

// Term j of item (kind, s, t); j < the item's number of terms.
DEV float proj_sample_term(const float* CR, const float* CL, const float* IR, const float* IL,
                           const float* __restrict__ P, int o, const float* crow, int m, int kind, int s, int t,
                           int j) {
  if (kind == 0) return CL[proj_off(j, m)] + CR[proj_off(m - 1 - j, m) + j] + marg_psi(P, o, crow, j + 1, 0);
  if (kind == 1) return IR[proj_off(j + 1, m) + s] + CR[proj_off(t - s - 1 - j, m) + s + 1 + j];
  if (kind == 2) return CL[proj_off(j, m) + s] + IL[proj_off(t - s - j, m) + s + j];
  return CR[proj_off(j, m) + s] + CL[proj_off(t - s - 1 - j, m) + s + j + 1];
}

// The draw of one item by a whole wave: the chosen term, -1 on a dead end.
template <int NS>
DEV int proj_sample_draw(const float* CR, const float* CL, const float* IR, const float* IL,
                         const float* __restrict__ P, int o, const float* crow, int m, int kind, int s, int t, int cnt,
                         float u, int lane) {
  float x[NS], q[NS];
  float M = MARG_NEG;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int j = lane + 64 * i;
    x[i] = j < cnt ? proj_sample_term(CR, CL, IR, IL, P, o, crow, m, kind, s, t, j) : MARG_NEG;
    M = fmaxf(M, x[i]);
  }
  for (int w = 32; w >= 1; w >>= 1) M = fmaxf(M, __shfl_xor(M, w));
  if (M == MARG_NEG) return -1;
#pragma unroll
  for (int i = 0; i < NS; ++i) q[i] = (x[i] == MARG_NEG) ? 0.f : expf(x[i] - M);
  return proj_sample_pick<NS>(q, u, lane);
}

// One sample by one wave over the filled tables: the heads by node into hd[0 ..
// n-1] (every lane writes the same values).  Returns 1, or 2 on a dead end.
DEV int proj_sample_walk(const float* tab, const float* __restrict__ P, int o, int n, int m, int lo, int single_root,
                         const float* crow, uint32_t k0, uint32_t k1, int g, int smp, int* hd, int* stk, int lane) {
  const int tri = PROJ_TRI(m);
  const float* CR = tab;
  const float* CL = tab + tri;
  const float* IR = tab + 2 * tri;
  const float* IL = tab + 3 * tri;
  for (int i = lane; i < n; i += 64) hd[i] = -1;
  int sp = 0;
#define PROJ_SAMPLE_PUSH(kind_, s_, t_)                              \
  do {                                                               \
    if ((s_) < (t_)) {                                               \
      if (sp >= PROJ_SAMPLE_STACK) return 2;                         \
      stk[sp++] = ((kind_) << 16) | ((s_) << 8) | (t_);              \
    }                                                                \
  } while (0)
  if (single_root) stk[sp++] = 0;
  else PROJ_SAMPLE_PUSH(1, 0, m - 1);
  for (int budget = 2 * m; sp > 0; --budget) {
    if (budget <= 0) return 2;  // (a derivation has at most 2 m - 1 items)
    const int item = stk[--sp];
    const int kind = item >> 16, s = (item >> 8) & 255, t = item & 255;
    const int cnt = kind == 0 ? m : t - s;
    const uint4 w = philox4x32_10(make_uint4((uint32_t)item, (uint32_t)smp, (uint32_t)g, PROJ_SAMPLE_STREAM), k0, k1);
    const float u = (float)(w.x >> 8) * 0x1p-24f;
    const int j = cnt <= 64 ? proj_sample_draw<1>(CR, CL, IR, IL, P, o, crow, m, kind, s, t, cnt, u, lane)
                            : proj_sample_draw<TREE_MAXV / 64>(CR, CL, IR, IL, P, o, crow, m, kind, s, t, cnt, u, lane);
    if (j < 0 || j >= cnt) return 2;
    if (kind == 0) {
      hd[1 + j] = 0;
      PROJ_SAMPLE_PUSH(2, 0, j);
      PROJ_SAMPLE_PUSH(1, j, m - 1);
    } else if (kind == 1) {
      const int r = s + 1 + j;
      PROJ_SAMPLE_PUSH(3, s, r);
      PROJ_SAMPLE_PUSH(1, r, t);
    } else if (kind == 2) {
      const int r = s + j;
      PROJ_SAMPLE_PUSH(2, s, r);
      PROJ_SAMPLE_PUSH(4, r, t);
    } else {
      const int r = s + j;
      if (kind == 3) hd[lo + t] = lo + s;
      else hd[lo + s] = lo + t;
      PROJ_SAMPLE_PUSH(1, s, r);
      PROJ_SAMPLE_PUSH(2, r + 1, t);
    }
  }
#undef PROJ_SAMPLE_PUSH
  return 1;
}

// The chunk's samples, a wave each: walks (st = 1) or the pass-through rows,
// and the outputs of every sample.  lg: ln Z of the graph.
template <int CHUNK>
DEV void proj_sample_chunk(const float* tab, const float* __restrict__ P, int o, int v, int n, int m, int lo,
                           int single_root, const float* crow, float lg, int st, uint32_t k0, uint32_t k1, int g, int K,
                           int first, int* hd, int* stk, int* __restrict__ heads, float* __restrict__ log_prob,
                           int* __restrict__ status, int lane, int wave) {
  const int last = min(K, first + CHUNK);
  for (int smp = first + wave; smp < last; smp += 4) {
    const int ss = st == 1 ? proj_sample_walk(tab, P, o, n, m, lo, single_root, crow, k0, k1, g, smp, hd, stk, lane)
                           : st;
    const long at = (long)g * K + smp;
    // the words' ln p into the stack's row (empty, or given up), then summed in word order
    for (int i = lane; i < v; i += 64) {
      const bool word = ss == 1 && i >= 1 && i < n;
      const int h = word ? hd[i] : -1;
      heads[at * v + i] = h;
      if (word) stk[i] = __float_as_int(h >= 0 ? logf(P[(long)i * o + h]) : 0.f);
    }
    __builtin_amdgcn_wave_barrier();  // (the wave's own LDS writes, in order)
    if (lane == 0) {
      double acc = 0.0;
      if (ss == 1)
        for (int i = 1; i < n; ++i) acc += (double)__int_as_float(stk[i]);
      log_prob[at] = ss == 1 ? (float)(acc - (double)lg) : -INFINITY;
      status[at] = ss;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// probs [b][v][o], n_nodes [b], heads [b][K][v], log_prob / status [b][K], logz
// [b] or NULL; ws: ws_stride floats per workgroup for the graphs with n >
// PROJ_SAMPLE_LDS_MAXN.  grid = b * chunks, chunks = ceil(K / CHUNK), block =
// 256.  (A template: its code is emitted after every kernel that was there
// before it, so those keep their places in the code object.)
template <int CHUNK>
__global__ void __launch_bounds__(256) k_projective_sample(const float* __restrict__ probs, int o,
                                                           const int* __restrict__ n_nodes, int v, int single_root,
                                                           int K, int chunks, uint32_t k0, uint32_t k1,
                                                           int* __restrict__ heads, float* __restrict__ log_prob,
                                                           int* __restrict__ status, float* __restrict__ logz,
                                                           float* ws, long ws_stride) {
  const int g = blockIdx.x / chunks, chunk = blockIdx.x - g * chunks, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int n = tree_node_count(n_nodes[g], v, o);
  const float* __restrict__ P = probs + (long)g * v * o;
  __shared__ float tab[4 * PROJ_TRI(PROJ_SAMPLE_LDS_MAXN)];
  __shared__ float crow[TREE_MAXV], zs[2];
  __shared__ int stk[4][PROJ_SAMPLE_STACK], hd[4][TREE_MAXV];

  int st = 0;
  const int lo = single_root ? 1 : 0, m = n - lo;
  // tables in LDS or in the workspace by the graph's own n
  const float* const T = n <= PROJ_SAMPLE_LDS_MAXN ? tab : ws + (long)blockIdx.x * ws_stride;
  if (n >= 2) {
    if (marg_crow(P, o, n, crow, tid)) st = 2;  // a word without an allowed arc
    else if (n <= PROJ_SAMPLE_LDS_MAXN) st = marg_inside(tab, P, o, n, m, lo, single_root, crow, zs, tid);
    else st = marg_inside(ws + (long)blockIdx.x * ws_stride, P, o, n, m, lo, single_root, crow, zs, tid);
  }
  const float lg = st == 1 ? zs[1] : st == 2 ? MARG_NEG : 0.f;
  if (logz && chunk == 0 && tid == 0) logz[g] = lg;
  proj_sample_chunk<CHUNK>(T, P, o, v, n, m, lo, single_root, crow, lg, st, k0, k1, g, K, chunk * CHUNK, hd[wave],
                           stk[wave], heads, log_prob, status, lane, wave);
}
