// k_tree_sample.h -- dependency trees drawn on the device from the distribution
// whose arc marginals k_lapl.h computes: the weight of a tree is the product of
// its words' head probabilities, crossing arcs included.  Conditional
// (ancestral) sampling on the matrix-tree inverse (the determinantal view of
// spanning trees, e.g. Colbourn, Myrvold & Neufeld 1996, on Koo et al. 2007's
// matrices); no random walk, so every loop is bounded by a function of n.  Host
// form: evaluation.py tree_sample_arrays.
//
// Per (graph, sample), with k_lapl.h's normalised potentials w(d, h) / r(d) and
// its allowed-arc rule:
//   multi-root:   A[h][d] = -w(d, h), A[d][d] = r(d) + sum_h w(d, h), B = A^-1.
//   single_root:  the one ROOT child rho is drawn first from marg[.][0] (the
//                 caller's ggnn_tree_marginals of the same input), restricted
//                 to the words with an allowed ROOT arc that reach every word
//                 (lapl_root_ok on lapl_reach's bit rows: a structural mask,
//                 rounding noise in marg never chooses an impossible root).
//                 Then r'(d) = [d == rho] and word rho's word potentials are 0
//                 (lapl_build's rho form): the rest of the tree is an
//                 arborescence over the words rooted at rho, and rho has no
//                 step of its own.
// The words are walked in ascending order.  Word d:
//   masses   q_0 = r'(d) B[d][d],  q_h = w(d, h) (B[d][d] - B[d][h]), clamped at
//            0; 0 for an arc that is not allowed and for an h whose chain of
//            already fixed heads ends in d (top[h] == d: it would close a
//            cycle), so a returned sample is a tree by construction.  Row d's
//            scale cancels: the kernel uses p[d][h] scaled by the row's power
//            of two (exact) in w's place.
//   draw     u = (x >> 8) * 2^-24, x the first word of Philox4x32-10 at counter
//            (d, s, g, 0x40000000) (d = 0: the ROOT child's draw) under the
//            64-bit seed.  With inclusive prefix sums c_j in ascending column
//            order and S the last: the smallest j with q_j > 0 and c_j > u S,
//            the largest j with q_j > 0 if rounding leaves none.
//   update   cvec = B[:, d] - e_d - [h* > 0] B[:, h*], den = B[d][d] - [h* > 0]
//            B[d][h*], B <- B - cvec (x) B[d, :] / den (Sherman-Morrison: column
//            d of A becomes e_d - e_h*).
// S not > 0 or den not finite and positive: a numerical dead end, status 2.
//
// B stays in k_lapl.h's permuted storage, B[i][l] = S[sig[i]][sinv[l]]: row d
// is storage row sig[d], column h storage column sinv[h], e_d sits in storage
// row sig[d], and the update is the elimination's flat walk over S.  Per step:
// the first ceil(n / 64) waves each make the draw for themselves (lane l holds
// columns l, l + 64, l + 128, l + 192: the row of probs_head is read coalesced
// and was fetched during the previous step's update, row sig[d] of S is read
// along the row; four interleaved 6-step wave scans and the segments' totals
// added in order give c_j), stage cvec (a column at the odd stride LD: every
// bank once) and the scaled row, and write the next top[]; barrier; every
// thread updates; barrier.  top[] is double-buffered so that the waves that
// draw never read what another is writing.
//
// Side arrays in LaplShared fields that are dead after the inversion: top[2][]
// in pv, the sample's heads in csum.  One workgroup of 1024 threads per (graph,
// sample), no atomics, nothing between workgroups, every scan and reduction in
// a fixed order: sample s of graph g depends on (seed, g, s) alone and two
// launches give the same bytes.
#pragma once
#include <cfloat>

#include "k_lapl.h"

#define SAMPLE_LDS_MAXN LAPL_LDS_MAXN  // GGNN_SAMPLE_LDS_MAXN: no LDS beside k_tree_marginals' own
#define SAMPLE_MAX 4096                // GGNN_SAMPLE_MAX
#define SAMPLE_SEGS (TREE_MAXV / 64)

static_assert(sizeof(float) * TREE_MAXV >= 2 * sizeof(short) * TREE_MAXV, "top[2][] lies in LaplShared::pv");
static_assert(sizeof(float) == sizeof(int), "the heads lie in LaplShared::csum");

DEV float sample_uniform(uint32_t k0, uint32_t k1, int g, int s, int d) {
  const uint4 w = philox4x32_10(make_uint4((uint32_t)d, (uint32_t)s, (uint32_t)g, 0x40000000u), k0, k1);
  return (float)(w.x >> 8) * 0x1p-24f;
}

// One draw by a whole wave: q[t] is the mass of column lane + 64 t.  Returns the
// drawn column, -1 when the masses do not sum to > 0; the same in every lane.
DEV int sample_pick(const float (&q)[SAMPLE_SEGS], float u, int lane) {
  float run[SAMPLE_SEGS], c[SAMPLE_SEGS];
#pragma unroll
  for (int t = 0; t < SAMPLE_SEGS; ++t) run[t] = q[t];
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) {
#pragma unroll
    for (int t = 0; t < SAMPLE_SEGS; ++t) {
      const float up = __shfl_up(run[t], w);
      if (lane >= w) run[t] += up;
    }
  }
  float total = 0.f;
#pragma unroll
  for (int t = 0; t < SAMPLE_SEGS; ++t) {
    c[t] = total + run[t];
    total += __shfl(run[t], 63);
  }
  if (!(total > 0.f)) return -1;
  const float target = u * total;
#pragma unroll
  for (int t = 0; t < SAMPLE_SEGS; ++t) {
    const unsigned long long hit = __ballot(q[t] > 0.f && c[t] > target);
    if (hit) return 64 * t + __ffsll(hit) - 1;
  }
#pragma unroll
  for (int t = SAMPLE_SEGS - 1; t >= 0; --t) {
    const unsigned long long live = __ballot(q[t] > 0.f);
    if (live) return 64 * t + 63 - __clzll(live);
  }
  return -1;
}

// The walk over the words of one sample (S: the inverse as lapl_invert left it;
// rho: the ROOT child drawn before, 0 without single_root).  Returns 1 with the
// heads in sh.csum (as int, by node) and thread 0's *lp = sum ln p[d][head_d],
// or 2.  Called by the whole workgroup.
DEV int sample_walk(float* S, LaplShared& sh, const float* __restrict__ P, int o, int n, int rho, uint32_t k0,
                    uint32_t k1, int g, int s, double* lp, int tid) {
  const int lane = tid & 63;
  const int m = n - 1, LD = LAPL_LD(m);
  const int act = (n + 63) & ~63;  // whole waves
  short* const top = (short*)sh.pv;
  int* const hd = (int*)sh.csum;
  if (tid < TREE_MAXV) {
    top[tid] = (short)((tid == rho || tid >= n) ? 0 : tid);
    hd[tid] = (rho && tid == rho) ? 0 : -1;
  }
  double acc = rho ? (double)logf(P[(long)rho * o]) : 0.0;
  float pn[SAMPLE_SEGS];
  {
    const int d0 = rho == 1 ? 2 : 1;
#pragma unroll
    for (int t = 0; t < SAMPLE_SEGS; ++t) {
      const int j = lane + 64 * t;
      pn[t] = (tid < act && d0 < n && j < n) ? P[(long)d0 * o + j] : 0.f;
    }
  }
  __syncthreads();
  const int q_ = LAPL_THREADS / LD, rr = LAPL_THREADS - q_ * LD, cells = m * LD;
  const int i0 = tid / LD, j0 = tid - i0 * LD;
  int cur = 0;
  for (int d = 1; d < n; ++d) {
    if (d == rho) continue;
    const int dp = d - 1;
    int dn = d + 1;
    if (dn == rho) ++dn;
    if (tid < act) {
      const short* const tc = top + cur * TREE_MAXV;
      short* const tn = top + (cur ^ 1) * TREE_MAXV;
      const int rd = sh.sig[dp] * LD, cd = sh.sinv[dp], e = sh.cexp[dp];
      const float bdd = S[rd + cd];
      float q[SAMPLE_SEGS];
#pragma unroll
      for (int t = 0; t < SAMPLE_SEGS; ++t) {
        const int j = lane + 64 * t;
        const float p = pn[t];
        float x = 0.f;
        if (j < n && j != d && marg_allowed(p)) {
          const float w = ldexpf(p, -e);
          if (j == 0) x = rho ? 0.f : w * bdd;
          else if (tc[j] != d) x = w * (bdd - S[rd + sh.sinv[j - 1]]);
        }
        q[t] = x > 0.f ? x : 0.f;
      }
      const int hs = sample_pick(q, sample_uniform(k0, k1, g, s, d), lane);
      bool dead = hs < 0;
      int ch = 0;
      float den = 0.f;
      if (!dead) {
        den = bdd;
        if (hs > 0) {
          ch = sh.sinv[hs - 1];
          den -= S[rd + ch];
        }
        dead = !(den > 0.f && den <= FLT_MAX);
      }
      if (!dead) {
        if (tid < m) {
          float c = S[tid * LD + cd] - (tid * LD == rd ? 1.f : 0.f);
          if (hs > 0) c -= S[tid * LD + ch];
          sh.col[tid] = c;
          sh.prow[tid] = S[rd + tid] / den;
        }
        if (tid < n) tn[tid] = tc[tid] == d ? (short)(hs > 0 ? tc[hs] : 0) : tc[tid];
        const int seg = hs >> 6;
        const float mine = seg == 0 ? pn[0] : seg == 1 ? pn[1] : seg == 2 ? pn[2] : pn[3];
        const float ph = __shfl(mine, hs & 63);
        if (tid == 0) {
          hd[d] = hs;
          acc += (double)logf(ph);
        }
      }
      if (tid == 0) sh.ctl[0] = dead;
    }
    __syncthreads();
    if (sh.ctl[0]) return 2;  // (the same for every thread)
    if (dn >= n) break;       // the last word: nothing left to condition
    if (tid < act) {          // the next word's row, under the update
#pragma unroll
      for (int t = 0; t < SAMPLE_SEGS; ++t) {
        const int j = lane + 64 * t;
        pn[t] = j < n ? P[(long)dn * o + j] : 0.f;
      }
    }
    for (int x = tid, i = i0, j = j0; x < cells; x += LAPL_THREADS) {
      if (j < m) S[x] = fmaf(-sh.col[i], sh.prow[j], S[x]);
      i += q_;
      j += rr;
      if (j >= LD) {
        j -= LD;
        ++i;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
  *lp = acc;
  return 1;
}

// One sample with its matrix at S (LDS or global).
DEV int sample_graph(float* S, LaplShared& sh, const float* __restrict__ P, int o, int n, int rho, uint32_t k0,
                     uint32_t k1, int g, int s, double* lp, int tid) {
  lapl_build(S, sh, P, o, n, 0, rho, tid);
  if (lapl_invert(S, sh, n, tid) != 1) return 2;
  return sample_walk(S, sh, P, o, n, rho, k0, k1, g, s, lp, tid);
}

// probs / marg [b][v][o], n_nodes / logz / marg_status [b] (ggnn_tree_marginals'
// outputs for the same probs, n_nodes and single_root; marg is read with
// single_root only), heads [b][K][v], log_prob / status [b][K]; ws: ws_stride
// floats per (graph, sample) for the graphs with n > SAMPLE_LDS_MAXN.  grid = b
// * K, block = LAPL_THREADS.  LDS: k_tree_marginals' arrays (163,272 B as laid
// out here).
__global__ void __launch_bounds__(LAPL_THREADS) k_tree_sample(const float* __restrict__ probs, int o,
                                                              const int* __restrict__ n_nodes, int v, int single_root,
                                                              const float* __restrict__ marg,
                                                              const float* __restrict__ logz,
                                                              const int* __restrict__ marg_status, int K, uint32_t k0,
                                                              uint32_t k1, int* __restrict__ heads,
                                                              float* __restrict__ log_prob, int* __restrict__ status,
                                                              float* ws, long ws_stride) {
  const int g = blockIdx.x / K, s = blockIdx.x - g * K, tid = threadIdx.x;
  const int n = tree_node_count(n_nodes[g], v, o);
  const long base = (long)g * v * o;
  const float* __restrict__ P = probs + base;
  __shared__ float mat[LAPL_MAT_FLOATS];
  __shared__ LaplShared sh;

  int st = n >= 2 ? marg_status[g] : 0;
  double lp = 0.0;
  if (st == 1) {
    int rho = 0;
    if (single_root) {  // the ROOT child
      const unsigned* R = lapl_reach((unsigned*)mat, P, o, n, tid);
      const bool good = lapl_root_ok(R, P, o, n, 1, tid);
      if (tid < TREE_MAXV) sh.col[tid] = good ? fmaxf(marg[base + (long)tid * o], 0.f) : 0.f;
      __syncthreads();
      if (tid < 64) {
        float q[SAMPLE_SEGS];
#pragma unroll
        for (int t = 0; t < SAMPLE_SEGS; ++t) q[t] = sh.col[tid + 64 * t];
        const int j = sample_pick(q, sample_uniform(k0, k1, g, s, 0), tid);
        if (tid == 0) sh.ctl[3] = j;
      }
      __syncthreads();
      rho = sh.ctl[3];
      if (rho < 1) st = 2;
    }
    if (st == 1) {
      if (n <= SAMPLE_LDS_MAXN)  // matrix in LDS or in the workspace by the graph's own n
        st = sample_graph(mat, sh, P, o, n, rho, k0, k1, g, s, &lp, tid);
      else
        st = sample_graph(ws + (long)blockIdx.x * ws_stride, sh, P, o, n, rho, k0, k1, g, s, &lp, tid);
    }
  }
  const long at = (long)g * K + s;
  const int* const hd = (const int*)sh.csum;
  for (int i = tid; i < v; i += LAPL_THREADS) heads[at * v + i] = (st == 1 && i >= 1 && i < n) ? hd[i] : -1;
  if (tid == 0) {
    log_prob[at] = st == 1 ? (float)(lp - (double)logz[g]) : -INFINITY;
    status[at] = st;
  }
}
