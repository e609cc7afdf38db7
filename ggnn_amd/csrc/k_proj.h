// k_proj.h -- projective decoding on the device (btb task): a post-pass on
// k_heads_decode's pred that leaves a graph alone when its arg-max heads
// already are a projective dependency tree and otherwise replaces them with
// the best projective tree of the integer head scores (Eisner's O(n^3) span
// dynamic programme).  Host form: evaluation.py projective_decode_arrays (the
// same formulation, length by length).
//
// Graph g, n = its node count.  Positions p = 0..m-1 stand for the nodes
// lo..lo+m-1: with single_root lo = 1, m = n - 1 (the words alone; ROOT's one
// arc is added at the end), without it lo = 0, m = n (node 0 is the leftmost
// position and never a dependent).  Four tables over spans s <= t:
//   CR[s][t]  complete, headed at s        CL[s][t]  complete, headed at t
//   IR[s][t]  incomplete, arc s -> t       IL[s][t]  incomplete, arc t -> s
//   base      = max_{s<=r<t}  CR[s][r] + CL[r+1][t]
//   IR[s][t]  = base + score(word t takes head s)     (allowed arcs only)
//   IL[s][t]  = base + score(word s takes head t)
//   CR[s][t]  = max_{s<r<=t}  IR[s][r] + CR[r][t]
//   CL[s][t]  = max_{s<=r<t}  CL[s][r] + IL[r][t]
// single_root: max_r CL[0][r] + CR[r][m-1] + score(word r+1 takes ROOT);
// otherwise CR[0][m-1].  A span without a derivation holds PROJ_NEG = -2^30
// exactly: the range check below keeps every real total strictly inside
// (-2^30, 2^30), proj_add never adds to a PROJ_NEG, so nothing wraps and the
// sentinel is never mistaken for a total.
//
// Layout: every table is packed by diagonals, entry (d = t - s, s) at
// d * m - d * (d - 1) / 2 + s, so the spans of one length are contiguous.  A
// length with `spans` spans gives each span G = 64 / spw lanes of a wave (spw
// = spans per wave, the power of two >= spans / 4); lane = q * spw + span, so
// the 32 lanes of an LDS access group read runs of min(spw, 32) consecutive
// dwords of one diagonal (operand 1) and of another (operand 2): conflict-free
// for the lengths that carry the work (spans >= 128: one run of 32), short
// runs at pseudo-random offsets for the long spans.  The G partial maxima are
// combined by a butterfly (decode_first_max's pattern).  The incomplete spans
// of a length are finished before its complete spans: two barriers per length.
//
// No split point is stored.  The walk-back (one wave, an explicit stack, no
// recursion) finds the smallest split of each of the < 2n spans on the path
// again by a ballot over the candidates that reach the span's value; pending
// spans have disjoint interiors, so the stack holds fewer than n entries.
//
// Graphs with n <= PROJ_LDS_MAXN keep the tables in LDS (8 m (m + 1) bytes,
// 132,096 at m = 128), larger ones in the caller's workspace (per graph, L2).
// One workgroup of 256 threads per graph, no atomics, nothing passes between
// workgroups, every loop is bounded by n, all choices are "smallest index
// wins": two launches give the same bytes.
#pragma once
#include "ggnn_common.h"
#include "k_tree.h"

#define PROJ_LDS_MAXN 128  // GGNN_PROJ_LDS_MAXN
#define PROJ_NEG (-(1 << 30))
#define PROJ_TRI(m) ((m) * ((m) + 1) / 2)
#define PROJ_STACK 512

DEV int proj_add(int a, int b) { return (a == PROJ_NEG || b == PROJ_NEG) ? PROJ_NEG : a + b; }
DEV int proj_off(int d, int m) { return d * m - ((d * (d - 1)) >> 1); }
DEV int proj_wave_max(int x, int from) {
  for (int w = 32; w >= from; w >>= 1) x = max(x, __shfl_xor(x, w));
  return x;
}
// the smallest lane with `hit`, -1 without one (wave-uniform)
DEV int proj_first(bool hit) {
  const unsigned long long mask = __ballot(hit);
  return mask ? __ffsll((long long)mask) - 1 : -1;
}

// Fills the four tables of one graph (tab: 4 * PROJ_TRI(m) ints, LDS or
// global) and walks the optimum back into nh[lo..lo+m-1] (and ROOT's child).
// Returns 1 with nh written, 2 when no projective tree exists.  Called by
// the whole workgroup.
DEV int proj_solve(int* tab, const int* __restrict__ S, int o, int m, int lo, int single_root, int* nh, int* stk,
                   int* flag, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const int tri = PROJ_TRI(m);
  int* TR = tab;
  int* TL = tab + tri;
  int* UR = tab + 2 * tri;
  int* UL = tab + 3 * tri;
  for (int s = tid; s < m; s += 256) TR[s] = TL[s] = 0;
  if (tid == 0) *flag = 0;
  __syncthreads();
  for (int L = 1; L < m; ++L) {
    const int spans = m - L, oL = proj_off(L, m);
    int lg = 0;  // spans per wave = 2^lg >= spans / 4
    for (; lg < 6 && (4 << lg) < spans; ++lg) {
    }
    const int spw = 1 << lg, G = 64 >> lg;
    const int s = wave * spw + (lane & (spw - 1)), q = lane >> lg;
    const bool live = s < spans;
    // incomplete spans: the best pair of facing complete spans, then the arc
    int best = PROJ_NEG;
    if (live)
      for (int k = q; k < L; k += G)
        best = max(best, proj_add(TR[proj_off(k, m) + s], TL[proj_off(L - 1 - k, m) + s + k + 1]));
    best = proj_wave_max(best, spw);
    if (live && q == 0) {
      const int ws = lo + s, wt = ws + L;  // wt >= 1
      const int a = S[(long)wt * o + ws];
      const int c = ws >= 1 ? S[(long)ws * o + wt] : TREE_FORBIDDEN;
      UR[oL + s] = (best != PROJ_NEG && a != TREE_FORBIDDEN) ? best + a : PROJ_NEG;
      UL[oL + s] = (best != PROJ_NEG && c != TREE_FORBIDDEN) ? best + c : PROJ_NEG;
    }
    __syncthreads();
    // complete spans (k = L - 1 reads the incomplete span just written)
    int br = PROJ_NEG, bl = PROJ_NEG;
    if (live)
      for (int k = q; k < L; k += G) {
        br = max(br, proj_add(UR[proj_off(k + 1, m) + s], TR[proj_off(L - 1 - k, m) + s + k + 1]));
        bl = max(bl, proj_add(TL[proj_off(k, m) + s], UL[proj_off(L - k, m) + s + k]));
      }
    br = proj_wave_max(br, spw);
    bl = proj_wave_max(bl, spw);
    if (live && q == 0) {
      TR[oL + s] = br;
      TL[oL + s] = bl;
    }
    __syncthreads();
  }

  // ---- the walk-back: wave 0, every value below is wave-uniform
  if (wave == 0) {
    int sp = 0;
    bool bad = false;
#define PROJ_PUSH(type_, s_, t_)                                    \
  do {                                                              \
    if ((s_) != (t_) || (type_) >= 2) {                             \
      if (sp < PROJ_STACK) stk[sp] = ((type_) << 16) | ((s_) << 8) | (t_); \
      else bad = true;                                              \
      ++sp;                                                         \
    }                                                               \
  } while (0)
    if (single_root) {
      int best = PROJ_NEG;
      for (int p = lane; p < m; p += 64) {
        const int a = S[(long)(p + 1) * o];
        const int c = proj_add(TL[proj_off(p, m)], TR[proj_off(m - 1 - p, m) + p]);
        best = max(best, (a != TREE_FORBIDDEN && c != PROJ_NEG) ? c + a : PROJ_NEG);
      }
      best = proj_wave_max(best, 1);
      int root = -1;
      if (best != PROJ_NEG)
        for (int pb = 0; pb < m && root < 0; pb += 64) {
          const int p = pb + lane;
          bool hit = false;
          if (p < m) {
            const int a = S[(long)(p + 1) * o];
            const int c = proj_add(TL[proj_off(p, m)], TR[proj_off(m - 1 - p, m) + p]);
            hit = a != TREE_FORBIDDEN && c != PROJ_NEG && c + a == best;
          }
          const int f = proj_first(hit);
          if (f >= 0) root = pb + f;
        }
      if (root < 0) {
        bad = true;
      } else {
        if (lane == 0) nh[lo + root] = 0;
        PROJ_PUSH(1, 0, root);
        PROJ_PUSH(0, root, m - 1);
      }
    } else {
      if (TR[proj_off(m - 1, m)] == PROJ_NEG) bad = true;
      else PROJ_PUSH(0, 0, m - 1);
    }
    for (int budget = 4 * m + 8; sp > 0 && !bad && budget > 0; --budget) {
      const int item = stk[--sp];
      const int type = item >> 16, s = (item >> 8) & 255, t = item & 255, L = t - s;
      int target;
      if (type == 0) target = TR[proj_off(L, m) + s];
      else if (type == 1) target = TL[proj_off(L, m) + s];
      else if (type == 2) target = UR[proj_off(L, m) + s] - S[(long)(lo + t) * o + lo + s];
      else target = UL[proj_off(L, m) + s] - S[(long)(lo + s) * o + lo + t];
      if (type == 2 && lane == 0) nh[lo + t] = lo + s;
      if (type == 3 && lane == 0) nh[lo + s] = lo + t;
      int found = -1;
      for (int kb = 0; kb < L && found < 0; kb += 64) {
        const int k = kb + lane;
        int c = PROJ_NEG;
        if (k < L) {
          if (type == 0) c = proj_add(UR[proj_off(k + 1, m) + s], TR[proj_off(L - 1 - k, m) + s + k + 1]);
          else if (type == 1) c = proj_add(TL[proj_off(k, m) + s], UL[proj_off(L - k, m) + s + k]);
          else c = proj_add(TR[proj_off(k, m) + s], TL[proj_off(L - 1 - k, m) + s + k + 1]);
        }
        const int f = proj_first(c != PROJ_NEG && c == target);
        if (f >= 0) found = kb + f;
      }
      if (found < 0) {
        bad = true;
      } else if (type == 0) {
        PROJ_PUSH(2, s, s + found + 1);
        PROJ_PUSH(0, s + found + 1, t);
      } else if (type == 1) {
        PROJ_PUSH(1, s, s + found);
        PROJ_PUSH(3, s + found, t);
      } else {
        PROJ_PUSH(0, s, s + found);
        PROJ_PUSH(1, s + found + 1, t);
      }
    }
#undef PROJ_PUSH
    if ((bad || sp > 0) && lane == 0) *flag = 1;
  }
  __syncthreads();
  return *flag ? 2 : 1;
}

// scores [b][v][o], n_nodes [b], pred [b][v][2] in/out, gold [b][v][2] and
// counts [b][DECODE_COUNTS] both or neither, status [b]; ws: ws_stride ints
// per graph for the graphs with n > PROJ_LDS_MAXN.  grid = b, block = 256.
__global__ void __launch_bounds__(256) k_projective_decode(const int* __restrict__ scores, int o,
                                                           const int* __restrict__ n_nodes, int v, int single_root,
                                                           int* __restrict__ pred, const int* __restrict__ gold,
                                                           int* __restrict__ counts, int* __restrict__ status,
                                                           int* ws, long ws_stride) {
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = tree_node_count(n_nodes[g], v, o);
  const long base = (long)g * v;
  const int* __restrict__ S = scores + base * o;
  if (n < 2) {
    if (tid == 0) status[g] = 0;
    return;
  }
  const int K = tree_doublings(n);
  __shared__ int tab[4 * PROJ_TRI(PROJ_LDS_MAXN)];
  __shared__ int jp[TREE_MAXV], alo[TREE_MAXV], ahi[TREE_MAXV], nh[TREE_MAXV], stk[PROJ_STACK], wmax[4], flag;

  // ---- the fast path: pred's heads already are a projective tree
  const bool word = tid > 0 && tid < n;
  TreePred t = tree_pred_arc(pred, S, o, base, n, jp, tid);
  alo[tid] = word && t.ok ? min(tid, t.h) : 0;
  ahi[tid] = word && t.ok ? max(tid, t.h) : 0;
  nh[tid] = -1;
  tree_pred_follow(t, n, K, jp, tid);
  if (t.is_tree && (!single_root || t.roots == 1)) {
    bool cross = false;
    if (word) {
      const int a = alo[tid], c = ahi[tid];
      for (int j = 1; j < n; ++j) cross |= a < alo[j] && alo[j] < c && c < ahi[j];
    }
    if (!__syncthreads_or(cross)) {
      if (tid == 0) status[g] = 0;
      return;
    }
  }

  // ---- the range check: S * (n - 1) < 2^30 keeps every span total in int32
  {
    int mx = 0;
    for (int i = 1 + wave; i < n; i += 4)
      for (int j = lane; j < n; j += 64) {
        const int s = S[(long)i * o + j];
        if (j != i && s != TREE_FORBIDDEN) mx = max(mx, s < 0 ? -s : s);
      }
    mx = proj_wave_max(mx, 1);
    if (lane == 0) wmax[wave] = mx;
    __syncthreads();
    mx = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
    if ((long long)mx * (n - 1) >= (1LL << 30)) {
      if (tid == 0) status[g] = 2;
      return;
    }
  }

  // ---- Eisner, tables in LDS or in the workspace by the graph's own n
  const int lo = single_root ? 1 : 0, m = n - lo;
  int st;
  if (n <= PROJ_LDS_MAXN) st = proj_solve(tab, S, o, m, lo, single_root, nh, stk, &flag, tid);
  else st = proj_solve(ws + (long)g * ws_stride, S, o, m, lo, single_root, nh, stk, &flag, tid);
  {
    const int hole = __syncthreads_or(st == 1 && word && (nh[tid] < 0 || nh[tid] >= n));
    if (st != 1 || hole) {
      if (tid == 0) status[g] = 2;
      return;
    }
    if (word) pred[(base + tid) * 2] = nh[tid];
    if (tid == 0) status[g] = 1;
  }
  tree_recount(gold, counts, pred, nh, n, v, base, g, tid);
}
