// k_marg.h -- projective arc marginals on the device (btb task): the
// sum-product twin of k_proj.h.  For every graph the posterior marginal of
// every arc "word i takes head j" under the distribution over projective
// dependency trees whose weight is the product of the words' head
// probabilities, the log of the total weight, and (when asked) the integer
// scores rint(marg * 2^20) whose Eisner optimum (k_proj.h) is the minimum
// Bayes risk tree.  Host form: evaluation.py projective_marginals_arrays (the
// same formulation, length by length).
//
// Positions, spans and the diagonal packing are k_proj.h's: p = 0..m-1 stand
// for the nodes lo..lo+m-1 (single_root: lo = 1), entry (d = t - s, s) of a
// table at d * m - d * (d - 1) / 2 + s.  psi(i, j) = ln p[i][j] - c[i] for an
// allowed arc (finite, > 0, 1 <= i < n, j < n, j != i), -inf otherwise, where
// c[i] is a per-word constant: every tree takes one arc per word, so the
// marginals do not depend on it and ln Z = ln Z' + sum c[i].  A first inside
// pass runs with c[i] = the largest ln p of word i's allowed arcs (a row's best
// arc has psi = 0) and gives ln Z'; then every c[i] grows by ln Z' / (n - 1)
// and both passes run on those potentials: a span's value no longer grows with
// its length (ln Z'' is about 0), so the tables hold the small numbers fp32 is
// precise on instead of sums of up to 255 logs of magnitude 87.
//
// Inside, by rising length (max -> log-sum-exp in k_proj.h's recurrences):
//   base      = lse_{s<=r<t}  CR[s][r] + CL[r+1][t]
//   IR[s][t]  = base + psi(t takes s)        IL[s][t] = base + psi(s takes t)
//   CR[s][t]  = lse_{s<r<=t}  IR[s][r] + CR[r][t]
//   CL[s][t]  = lse_{s<=r<t}  CL[s][r] + IL[r][t]
//   ln Z      = lse_r CL[0][r] + CR[r][m-1] + psi(r+1 takes ROOT)   (single_root)
//             = CR[0][m-1]                                          (otherwise)
// Outside, by falling length; the outside value of a span is gathered from the
// longer spans it is a part of (oB = outside of `base`):
//   oCR[s][t] = lse( lse_{a<s}  oCR[a][t]  + IR[a][s],     (right part of CR[a][t])
//                    lse_{u>t}  oB[s][u]   + CL[t+1][u],   (left part of base[s][u])
//                    [t = m-1]  CL[0][s] + psi(s+1 takes ROOT)  /  [span 0..m-1] 0 )
//   oCL[s][t] = lse( lse_{u>t}  oCL[s][u]  + IL[t][u],     (left part of CL[s][u])
//                    lse_{a<s}  oB[a][t]   + CR[a][s-1],   (right part of base[a][t])
//                    [s = 0]    CR[t][m-1] + psi(t+1 takes ROOT) )
//   oIR[s][t] = lse_{u>=t} oCR[s][u] + CR[t][u]            (left part of CR[s][u])
//   oIL[s][t] = lse_{a<=s} oCL[a][t] + CL[a][s]            (right part of CL[a][t])
//   oB[s][t]  = lse( oIR + psi(t takes s), oIL + psi(s takes t) )
//   marg(t takes s) = exp(IR[s][t] + oIR[s][t] - ln Z), marg(s takes t) alike
// (ln Z here: that of the potentials the tables were filled with)
// oIR / oIL are used where they are made, so SEVEN tables are stored (CR, CL,
// IR, IL, oCR, oCL, oB): 14 m (m + 1) bytes, 161,784 at m = MARG_LDS_MAXN =
// 107, which with c[] fills the 160 KiB of a CU.  Larger graphs keep the
// tables in the caller's workspace (per graph, L2).
//
// Work mapping is k_proj.h's: a length with `spans` spans gives each span G =
// 64 / spw lanes of a wave, lane = q * spw + span, the span's terms strided by
// G.  Every sum above walks by DISTANCE from the span (a = s - 1 - j, u = t +
// 1 + j), so at one step the lanes of a q read one diagonal at consecutive
// offsets in both passes: runs of min(spw, 32) consecutive dwords per LDS
// access group, conflict-free for spans >= 128 as in the inside pass.  Each
// lane keeps a running (max, sum of exp(x - max)); the G lanes are combined by
// two butterflies in a fixed order, the maximum first, then the rescaled sums.
// -inf marks a span without a derivation and is never subtracted.
//
// One workgroup of 256 threads per graph, two barriers per length and pass,
// no atomics, nothing passes between workgroups, every loop is bounded by n,
// every reduction has a fixed order: two launches give the same bytes.
#pragma once
#include <cfloat>

#include "ggnn_common.h"
#include "k_proj.h"
#include "k_tree.h"

#define MARG_LDS_MAXN 107  // GGNN_MARG_LDS_MAXN
#define MARG_TABLES 7
#define MARG_NEG (-INFINITY)
#define MARG_SCALE 1048576.f  // 2^20

// x joins a running log-sum-exp (mx = the maximum so far, sm = sum exp(. - mx))
DEV void marg_acc(float& mx, float& sm, float x) {
  if (x > mx) {
    sm = (mx == MARG_NEG) ? 1.f : sm * expf(mx - x) + 1.f;
    mx = x;
  } else if (x != MARG_NEG) {
    sm += expf(x - mx);
  }
}
// the log-sum-exp of the accumulators of the lanes that differ in the lane
// bits >= from (from = 1: the whole wave); every lane of the wave calls it
DEV float marg_finish(float mx, float sm, int from) {
  float M = mx;
  for (int w = 32; w >= from; w >>= 1) M = fmaxf(M, __shfl_xor(M, w));
  float s = (mx == MARG_NEG) ? 0.f : sm * expf(mx - M);
  for (int w = 32; w >= from; w >>= 1) s += __shfl_xor(s, w);
  return (M == MARG_NEG) ? MARG_NEG : M + logf(s);
}
DEV bool marg_allowed(float p) { return p > 0.f && p <= FLT_MAX; }  // (false for a NaN)
// psi(node i takes node j), j != i
DEV float marg_psi(const float* __restrict__ P, int o, const float* crow, int i, int j) {
  if (i < 1) return MARG_NEG;
  const float p = P[(long)i * o + j];
  return marg_allowed(p) ? logf(p) - crow[i] : MARG_NEG;
}
DEV void marg_store(float* __restrict__ marg, int* __restrict__ scores, long at, float x, float z) {
  const float val = (x == MARG_NEG) ? 0.f : fminf(1.f, expf(x - z));
  marg[at] = val;
  if (scores) scores[at] = (int)rintf(val * MARG_SCALE);
}

// c[i] of one graph (n >= 2): the largest allowed ln p of every word's row, a
// wave per row.  Returns whether a word has no allowed arc (the same for every
// thread).  Called by the whole workgroup; ends in a barrier.
DEV bool marg_crow(const float* __restrict__ P, int o, int n, float* crow, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  bool empty = false;
  for (int i = 1 + wave; i < n; i += 4) {
    float mx = 0.f;
    for (int j = lane; j < n; j += 64) {
      const float p = P[(long)i * o + j];
      if (j != i && marg_allowed(p)) mx = fmaxf(mx, p);
    }
    for (int w = 32; w >= 1; w >>= 1) mx = fmaxf(mx, __shfl_xor(mx, w));
    if (lane == 0) crow[i] = mx > 0.f ? logf(mx) : 0.f;
    empty |= !(mx > 0.f);
  }
  if (tid == 0) crow[0] = 0.f;
  return __syncthreads_or(empty);
}

// The inside passes of one graph (tab: the four inside tables first, 4 *
// PROJ_TRI(m) floats, LDS or global).  Returns 1 with the tables filled on the
// shifted potentials (crow updated), zs[0] = their ln Z'' and zs[1] = ln Z of
// the graph's own potentials, 2 when ln Z is not finite.  Called by the whole
// workgroup; ends in a barrier.  Shared with k_proj_sample.h.
DEV int marg_inside(float* tab, const float* __restrict__ P, int o, int n, int m, int lo, int single_root,
                    float* crow, float* zs, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const int tri = PROJ_TRI(m);
  float* CR = tab;
  float* CL = tab + tri;
  float* IR = tab + 2 * tri;
  float* IL = tab + 3 * tri;
  // ---- inside, twice: the first pass finds ln Z' on psi = ln p - (the row's largest ln p); the second runs
  // on psi - ln Z' / (n - 1), every word giving up its share of ln Z', so that a span's value stays near 0
  // instead of growing with its length, where fp32 is coarse (ln Z'' is then about 0)
  float z = 0.f;
  for (int pass = 0; pass < 2; ++pass) {
    for (int s = tid; s < m; s += 256) CR[s] = CL[s] = 0.f;
    __syncthreads();
    for (int L = 1; L < m; ++L) {
      const int spans = m - L, oL = proj_off(L, m);
      int lg = 0;  // spans per wave = 2^lg >= spans / 4
      for (; lg < 6 && (4 << lg) < spans; ++lg) {
      }
      const int spw = 1 << lg, G = 64 >> lg;
      const int s = wave * spw + (lane & (spw - 1)), q = lane >> lg;
      const bool live = s < spans;
      float bx = MARG_NEG, bs = 0.f;
      if (live)
        for (int k = q; k < L; k += G)
          marg_acc(bx, bs, CR[proj_off(k, m) + s] + CL[proj_off(L - 1 - k, m) + s + k + 1]);
      const float base = marg_finish(bx, bs, spw);
      if (live && q == 0) {
        const int ws = lo + s, wt = ws + L;
        IR[oL + s] = base + marg_psi(P, o, crow, wt, ws);
        IL[oL + s] = base + marg_psi(P, o, crow, ws, wt);
      }
      __syncthreads();
      float rx = MARG_NEG, rs = 0.f, lx = MARG_NEG, ls = 0.f;
      if (live)
        for (int k = q; k < L; k += G) {
          marg_acc(rx, rs, IR[proj_off(k + 1, m) + s] + CR[proj_off(L - 1 - k, m) + s + k + 1]);
          marg_acc(lx, ls, CL[proj_off(k, m) + s] + IL[proj_off(L - k, m) + s + k]);
        }
      const float cr = marg_finish(rx, rs, spw), cl = marg_finish(lx, ls, spw);
      if (live && q == 0) {
        CR[oL + s] = cr;
        CL[oL + s] = cl;
      }
      __syncthreads();
    }
    if (wave == 0) {  // ln Z of this pass's potentials
      float mx = MARG_NEG, sm = 0.f;
      if (single_root) {
        for (int p = lane; p < m; p += 64)
          marg_acc(mx, sm, CL[proj_off(p, m)] + CR[proj_off(m - 1 - p, m) + p] + marg_psi(P, o, crow, p + 1, 0));
      } else if (lane == 0) {
        marg_acc(mx, sm, CR[proj_off(m - 1, m)]);
      }
      const float zw = marg_finish(mx, sm, 1);
      if (lane == 0) zs[0] = zw;
    }
    __syncthreads();
    z = zs[0];
    if (!(z > MARG_NEG && z <= FLT_MAX)) return 2;  // no projective tree (the same for every thread)
    if (pass == 0) {
      const float share = z / (float)(n - 1);
      for (int i = 1 + tid; i < n; i += 256) crow[i] += share;
      __syncthreads();
    }
  }
  // ---- ln Z = ln Z'' + sum c[i] (wave 0, fixed order)
  if (wave == 0) {
    float c = 0.f;
    for (int i = 1 + lane; i < n; i += 64) c += crow[i];
    for (int w = 32; w >= 1; w >>= 1) c += __shfl_xor(c, w);
    if (lane == 0) zs[1] = z + c;
  }
  __syncthreads();
  if (!(fabsf(zs[1]) <= FLT_MAX)) return 2;
  return 1;
}

// The passes of one graph (tab: MARG_TABLES * PROJ_TRI(m) floats, LDS or
// global; marg / scores / logz point at the graph's own outputs).  Returns 1
// with the outputs written, 2 (nothing written) when ln Z is not finite.
// Called by the whole workgroup.
DEV int marg_solve(float* tab, const float* __restrict__ P, int o, int v, int n, int m, int lo, int single_root,
                   float* crow, float* zs, float* __restrict__ marg, int* __restrict__ scores,
                   float* __restrict__ logz, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const int tri = PROJ_TRI(m);
  float* CR = tab;
  float* CL = tab + tri;
  float* IR = tab + 2 * tri;
  float* IL = tab + 3 * tri;
  float* OR = tab + 4 * tri;
  float* OL = tab + 5 * tri;
  float* OB = tab + 6 * tri;
  if (marg_inside(tab, P, o, n, m, lo, single_root, crow, zs, tid) != 1) return 2;
  const float z = zs[0];
  if (tid == 0) *logz = zs[1];
  // ---- every arc starts as "not allowed"; the allowed ones are written once each below
  for (long x = tid; x < (long)v * o; x += 256) {
    marg[x] = 0.f;
    if (scores) scores[x] = TREE_FORBIDDEN;
  }
  __syncthreads();
  if (single_root)
    for (int p = tid; p < m; p += 256) {
      const float a = marg_psi(P, o, crow, p + 1, 0);
      if (a != MARG_NEG)
        marg_store(marg, scores, (long)(p + 1) * o, CL[proj_off(p, m)] + CR[proj_off(m - 1 - p, m) + p] + a, z);
    }
  // ---- outside
  for (int L = m - 1; L >= 1; --L) {
    const int spans = m - L, oL = proj_off(L, m);
    int lg = 0;
    for (; lg < 6 && (4 << lg) < spans; ++lg) {
    }
    const int spw = 1 << lg, G = 64 >> lg;
    const int s = wave * spw + (lane & (spw - 1)), q = lane >> lg, t = s + L;
    const bool live = s < spans;
    // complete spans: from the longer spans that start left of s or end right of t
    float rx = MARG_NEG, rs = 0.f, lx = MARG_NEG, ls = 0.f;
    if (live) {
      for (int j = q; j < s; j += G) {
        const int a = s - 1 - j, od = proj_off(L + 1 + j, m) + a;
        marg_acc(rx, rs, OR[od] + IR[proj_off(j + 1, m) + a]);
        marg_acc(lx, ls, OB[od] + CR[proj_off(j, m) + a]);
      }
      for (int j = q; t + 1 + j < m; j += G) {
        const int od = proj_off(L + 1 + j, m) + s;
        marg_acc(rx, rs, OB[od] + CL[proj_off(j, m) + t + 1]);
        marg_acc(lx, ls, OL[od] + IL[proj_off(j + 1, m) + t]);
      }
      if (q == 0) {
        if (single_root) {
          if (t == m - 1) marg_acc(rx, rs, CL[proj_off(s, m)] + marg_psi(P, o, crow, s + 1, 0));
          if (s == 0) marg_acc(lx, ls, CR[proj_off(m - 1 - t, m) + t] + marg_psi(P, o, crow, t + 1, 0));
        } else if (L == m - 1) {
          marg_acc(rx, rs, 0.f);
        }
      }
    }
    const float ocr = marg_finish(rx, rs, spw), ocl = marg_finish(lx, ls, spw);
    if (live && q == 0) {
      OR[oL + s] = ocr;
      OL[oL + s] = ocl;
    }
    __syncthreads();
    // incomplete spans (j = 0 reads the complete span just written), their arcs' marginals
    float ax = MARG_NEG, as = 0.f, cx = MARG_NEG, cs = 0.f;
    if (live) {
      for (int j = q; t + j < m; j += G) marg_acc(ax, as, OR[proj_off(L + j, m) + s] + CR[proj_off(j, m) + t]);
      for (int j = q; j <= s; j += G) marg_acc(cx, cs, OL[proj_off(L + j, m) + s - j] + CL[proj_off(j, m) + s - j]);
    }
    const float oir = marg_finish(ax, as, spw), oil = marg_finish(cx, cs, spw);
    if (live && q == 0) {
      const int ws = lo + s, wt = lo + t;
      const float wr = marg_psi(P, o, crow, wt, ws), wl = marg_psi(P, o, crow, ws, wt);
      const float br = oir + wr, bl = oil + wl, M = fmaxf(br, bl);
      OB[oL + s] = (M == MARG_NEG)
                       ? MARG_NEG
                       : M + logf((br == MARG_NEG ? 0.f : expf(br - M)) + (bl == MARG_NEG ? 0.f : expf(bl - M)));
      if (wr != MARG_NEG) marg_store(marg, scores, (long)wt * o + ws, IR[oL + s] + oir, z);
      if (wl != MARG_NEG) marg_store(marg, scores, (long)ws * o + wt, IL[oL + s] + oil, z);
    }
    __syncthreads();
  }
  return 1;
}

// probs [b][v][o], n_nodes [b], marg [b][v][o], logz [b], scores [b][v][o] or
// NULL, status [b]; ws: ws_stride floats per graph for the graphs with n >
// MARG_LDS_MAXN.  grid = b, block = 256.
__global__ void __launch_bounds__(256) k_projective_marginals(const float* __restrict__ probs, int o,
                                                              const int* __restrict__ n_nodes, int v,
                                                              int single_root, float* __restrict__ marg,
                                                              float* __restrict__ logz, int* __restrict__ scores,
                                                              int* __restrict__ status, float* ws, long ws_stride) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n = tree_node_count(n_nodes[g], v, o);
  const long base = (long)g * v * o;
  const float* __restrict__ P = probs + base;
  __shared__ float tab[MARG_TABLES * PROJ_TRI(MARG_LDS_MAXN)];
  __shared__ float crow[TREE_MAXV], zs[2];

  int st = 0;
  if (n >= 2) {
    if (marg_crow(P, o, n, crow, tid)) {
      st = 2;  // a word without an allowed arc
    } else {
      const int lo = single_root ? 1 : 0, m = n - lo;
      int* const S = scores ? scores + base : nullptr;
      // tables in LDS or in the workspace by the graph's own n
      if (n <= MARG_LDS_MAXN)
        st = marg_solve(tab, P, o, v, n, m, lo, single_root, crow, zs, marg + base, S, logz + g, tid);
      else
        st = marg_solve(ws + (long)g * ws_stride, P, o, v, n, m, lo, single_root, crow, zs, marg + base, S, logz + g,
                        tid);
    }
  }
  if (st != 1) {  // the graph passes through: the plain arg-max downstream
    for (long x = tid; x < (long)v * o; x += 256) {
      marg[base + x] = P[x];
      if (scores) scores[base + x] = TREE_FORBIDDEN;
    }
    if (tid == 0) logz[g] = st == 2 ? MARG_NEG : 0.f;
  }
  if (tid == 0) status[g] = st;
}

// conf[g][i] = marg[g][i][pred[g][i][0]], 0 where the predicted head is -1 or
// the row is 0 or >= n.  grid = ceil(b * v / 256), block = 256.
__global__ void __launch_bounds__(256) k_arc_confidence(const float* __restrict__ marg, int o,
                                                        const int* __restrict__ n_nodes, int b, int v,
                                                        const int* __restrict__ pred, float* __restrict__ conf) {
  const long x = (long)blockIdx.x * 256 + threadIdx.x;
  if (x >= (long)b * v) return;
  const int g = (int)(x / v), i = (int)(x % v);
  const int n = max(0, min(n_nodes[g], min(v, o)));
  const int h = pred[x * 2];
  conf[x] = (i >= 1 && i < n && h >= 0 && h < o) ? marg[x * o + h] : 0.f;
}
