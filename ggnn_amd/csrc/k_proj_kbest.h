// k_proj_kbest.h -- the K best projective dependency trees of the integer head
// scores, in order, on the device: k_proj.h's span dynamic programme with a
// sorted LIST of up to K entries per item instead of one value (Huang & Chiang
// 2005 in Eisner's formulation).  Host form: evaluation.py
// projective_kbest_arrays.
//
// Positions, lo / m, allowed arcs, the PROJ_NEG sentinel, the range rule and the
// packing by diagonals are k_proj.h's.  IR and IL of a span differ by the arc's
// score alone, so three lists per span are kept: CR, CL and the base BS = the
// pairs of facing complete spans; the two arc scores of the span lie beside
// them (AR: word t takes s, AL: word s takes t; TREE_FORBIDDEN = no such arc).
//   BS[s][t]  candidates (r, i, j), s <= r < t:  CR[s][r][i] + CL[r+1][t][j]
//   CR[s][t]  candidates (r, i, j), s < r <= t:  BS[s][r][i] + AR[s][r] + CR[r][t][j]
//   CL[s][t]  candidates (r, i, j), s <= r < t:  CL[s][r][i] + BS[r][t][j] + AL[r][t]
//   final     single_root: (p, i, j): CL[0][p][i] + CR[p][m-1][j] + score(p+1 takes ROOT);
//             otherwise CR[0][m-1]'s list
// A candidate exists when both entries exist and the arc is allowed.  A list is
// the first K candidates in the TOTAL ORDER: larger total first, then the smaller
// split, then the smaller first rank, then the smaller second rank.  As a
// 64-bit key, larger = earlier:
//   key = (total + 2^30) << 32 | (0xFFFFFFFF - (k << 8 | i << 4 | j))
// with k the split counted from the span's first candidate (k <= 254, ranks <=
// 15); a real total lies strictly inside (-2^30, 2^30), so a key is never 0 and
// 0 stands for "none".  0xFFFFFFFF minus the low word is the entry's
// back-pointer, stored beside its value: the walk-back never searches by value
// (with ties two ranks would find the same tree).  Candidate (k, i, j) has (i +
// 1)(j + 1) - 1 candidates of its split ahead of it, so only the pairs with (i
// + 1)(j + 1) <= K are looked at.
//
// Selection: K rounds of "the largest key below the last one taken".  A span's
// splits are spread over a lane group as in proj_solve (lane = q * spw + span,
// G = 64 / spw lanes per span); per round every lane finds the best key of its
// own splits and a butterfly over the group combines them.  Keys fall along
// every list, so a lane leaves a split at its first key that does not beat the
// lane's best so far, a first rank likewise, and a second rank at the first key
// below the bound: a round costs a few reads per split, not K log K.  The two
// list heads and the arc score of KBEST_BATCH splits are loaded together before
// any of them is looked at (three independent loads per split in flight, not
// three dependent ones: the global tier is L2 latency).  The result is a
// function of the inputs alone: every choice is a maximum of distinct keys.
//
// Layout: rank-major, V[r * tri + (diagonal offset + s)]: the lanes of a group
// read runs of consecutive dwords of one diagonal whatever the rank (k_proj.h's
// banking argument, rank by rank).  Per span 6 K + 2 ints: three value lists,
// three back-pointer lists, two arc scores.  A graph whose PROJ_TRI(n) * (6 K +
// 2) ints fit KBEST_TAB_INTS keeps them in LDS (n <= 97 at K = 1, 73 at 2, 27
// at 16), a larger one in the caller's workspace (per graph, L2).
//
// The walk-back of rank k is one wave's work (ranks wave, wave + 4, ...): an
// explicit stack of (kind, rank, s, t) items in the wave's own LDS row, every
// lane holding the same values, so no barrier is needed.  Pending items have
// disjoint interiors and s < t: fewer than m are pending at once, and a
// derivation has at most 2 m - 1 items; an overflow, an exhausted budget, a
// split outside its span or a word left without a head make the graph status 2,
// never a write outside a buffer.  One workgroup of 256 threads per graph, no
// atomics, nothing between workgroups, every loop bounded by a function of n
// and K: two launches give the same bytes.
#pragma once
#include "k_proj.h"

#define KBEST_MAX 16          // GGNN_KBEST_MAX
#define KBEST_TAB_INTS 38400  // 150 KiB of tables in LDS
#define KBEST_STACK TREE_MAXV
#define KBEST_BATCH 4  // splits whose list heads a lane loads together
#define KBEST_SPAN_INTS(K) (6 * (K) + 2)
#define KBEST_LDS_BYTES (sizeof(int) * (KBEST_TAB_INTS + 4 * KBEST_STACK + 4 * TREE_MAXV + 2 * KBEST_MAX + 8))

static_assert(TREE_MAXV <= 256 && KBEST_MAX <= 16, "a back-pointer packs a split below 255 and two ranks below 16");
static_assert(KBEST_STACK >= TREE_MAXV - 1, "fewer than m items are pending");
static_assert(KBEST_LDS_BYTES <= 160 * 1024, "tables, four stacks, four head rows and the final list fit the LDS of a CU");

// whether a graph of n nodes keeps its tables in LDS at this K
DEV bool kbest_in_lds(int n, int K) { return PROJ_TRI(n) * KBEST_SPAN_INTS(K) <= KBEST_TAB_INTS; }

typedef unsigned long long kb_key;

DEV kb_key kbest_key(int total, int k, int i, int j) {
  return ((kb_key)(unsigned)(total + (1 << 30)) << 32) | (kb_key)(0xFFFFFFFFu - (unsigned)((k << 8) | (i << 4) | j));
}
DEV kb_key kbest_group_max(kb_key x, int from) {
  for (int w = 32; w >= from; w >>= 1) {
    const unsigned hi = (unsigned)__shfl_xor((int)(x >> 32), w), lo = (unsigned)__shfl_xor((int)(unsigned)x, w);
    const kb_key y = ((kb_key)hi << 32) | lo;
    x = y > x ? y : x;
  }
  return x;
}

// The tables of one graph: three value lists, three back-pointer lists (rank r
// of the span at packed index x: [r * tri + x]) and the two arc scores by span.
struct KBest {
  int *cr, *cl, *bs, *crb, *clb, *bsb, *ar, *al;
  int tri, m, K;
};
DEV KBest kbest_tables(int* tab, int m, int K) {
  KBest t;
  t.tri = PROJ_TRI(m);
  t.m = m;
  t.K = K;
  const int n = t.tri * K;
  t.cr = tab;
  t.cl = tab + n;
  t.bs = tab + 2 * n;
  t.crb = tab + 3 * n;
  t.clb = tab + 4 * n;
  t.bsb = tab + 5 * n;
  t.ar = tab + 6 * n;
  t.al = t.ar + t.tri;
  return t;
}

// The list of one item: KIND 0 BS, 1 CR, 2 CL of the span (L, s), 3 the final
// list under single_root (L = m splits, s = 0; S: the graph's scores).  The
// lanes q, q + G, ... of the span's group take the splits q, q + G, ...; `from`
// = the group's lowest butterfly distance (spw).  Lane q = 0 of a live span
// writes outv / outb[r * ostride + oidx] for every r < K (PROJ_NEG / 0 where
// the candidates run out).  Called by whole waves.
template <int KIND>
DEV void kbest_select(const KBest& T, const int* __restrict__ S, int o, int L, int s, int q, int G, int from,
                      bool live, int* outv, int* outb, int ostride, int oidx) {
  const int m = T.m, tri = T.tri, K = T.K;
  const int* const A0 = KIND == 0 ? T.cr : KIND == 1 ? T.bs : T.cl;  // the first / second child's lists
  const int* const B0 = KIND == 0 ? T.cl : KIND == 2 ? T.bs : T.cr;
  kb_key bound = ~(kb_key)0;
  for (int r = 0; r < K; ++r) {
    kb_key best = 0;
    if (live && bound != 0)
      for (int kb = q; kb < L; kb += KBEST_BATCH * G) {
        // the list heads and arc scores of KBEST_BATCH splits in flight together
        int ia[KBEST_BATCH], ib[KBEST_BATCH], arc[KBEST_BATCH], a0[KBEST_BATCH], b0[KBEST_BATCH];
#pragma unroll
        for (int u = 0; u < KBEST_BATCH; ++u) {
          const int k = kb + u * G;
          arc[u] = TREE_FORBIDDEN;
          a0[u] = b0[u] = PROJ_NEG;
          if (k < L) {
            if (KIND == 0) ia[u] = proj_off(k, m) + s, ib[u] = proj_off(L - 1 - k, m) + s + k + 1;
            else if (KIND == 1) ia[u] = proj_off(k + 1, m) + s, ib[u] = proj_off(L - 1 - k, m) + s + k + 1;
            else if (KIND == 2) ia[u] = proj_off(k, m) + s, ib[u] = proj_off(L - k, m) + s + k;
            else ia[u] = proj_off(k, m), ib[u] = proj_off(m - 1 - k, m) + k;
            arc[u] = KIND == 0 ? 0 : KIND == 1 ? T.ar[ia[u]] : KIND == 2 ? T.al[ib[u]] : S[(long)(k + 1) * o];
            a0[u] = A0[ia[u]];
            b0[u] = B0[ib[u]];
          }
        }
#pragma unroll
        for (int u = 0; u < KBEST_BATCH; ++u) {
          const int k = kb + u * G;
          if (arc[u] == TREE_FORBIDDEN || a0[u] == PROJ_NEG || b0[u] == PROJ_NEG) continue;
          for (int i = 0; i < K; ++i) {
            const int a = i ? A0[i * tri + ia[u]] : a0[u];
            if (a == PROJ_NEG) break;
            if (kbest_key(a + arc[u] + b0[u], k, i, 0) <= best) break;  // (every later key of the split is smaller)
            const int jn = K / (i + 1);
            for (int j = 0; j < jn; ++j) {
              const int b = j ? B0[j * tri + ib[u]] : b0[u];
              if (b == PROJ_NEG) break;
              const kb_key key = kbest_key(a + arc[u] + b, k, i, j);
              if (key <= best) break;
              if (key < bound) {
                best = key;
                break;
              }
            }
          }
        }
      }
    best = kbest_group_max(best, from);
    bound = best;
    if (live && q == 0) {
      outv[r * ostride + oidx] = best ? (int)(unsigned)(best >> 32) - (1 << 30) : PROJ_NEG;
      outb[r * ostride + oidx] = best ? (int)(0xFFFFFFFFu - (unsigned)best) : 0;
    }
  }
}

// Fills the tables of one graph (tab: PROJ_TRI(m) * KBEST_SPAN_INTS(K) ints, LDS
// or global) and the final list finv / finb[K].  Called by the whole workgroup;
// ends in a barrier.
DEV void kbest_fill(int* tab, const int* __restrict__ S, int o, int m, int lo, int single_root, int K, int* finv,
                    int* finb, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const KBest T = kbest_tables(tab, m, K);
  const int tri = T.tri;
  for (int x = tid; x < m * K; x += 256) {
    const int r = x / m, s = x - r * m;
    T.cr[r * tri + s] = T.cl[r * tri + s] = r ? PROJ_NEG : 0;
  }
  __syncthreads();
  for (int L = 1; L < m; ++L) {
    const int spans = m - L, oL = proj_off(L, m);
    int lg = 0;  // spans per wave = 2^lg >= spans / 4
    for (; lg < 6 && (4 << lg) < spans; ++lg) {
    }
    const int spw = 1 << lg, G = 64 >> lg;
    const int s = wave * spw + (lane & (spw - 1)), q = lane >> lg;
    const bool live = s < spans;
    if (live && q == 0) {
      const int ws = lo + s, wt = ws + L;  // wt >= 1
      T.ar[oL + s] = S[(long)wt * o + ws];
      T.al[oL + s] = ws >= 1 ? S[(long)ws * o + wt] : TREE_FORBIDDEN;
    }
    kbest_select<0>(T, S, o, L, s, q, G, spw, live, T.bs, T.bsb, tri, oL + s);
    __syncthreads();
    // complete spans (their last / first split reads the base list just written)
    kbest_select<1>(T, S, o, L, s, q, G, spw, live, T.cr, T.crb, tri, oL + s);
    kbest_select<2>(T, S, o, L, s, q, G, spw, live, T.cl, T.clb, tri, oL + s);
    __syncthreads();
  }
  if (single_root) {
    if (wave == 0) kbest_select<3>(T, S, o, m, 0, lane, 64, 1, true, finv, finb, 1, 0);
  } else {
    const int x = proj_off(m - 1, m);
    if (tid < K) {
      finv[tid] = T.cr[tid * tri + x];
      finb[tid] = 0;
    }
  }
  __syncthreads();
}

// The tree of final rank `rank` (it exists) by one wave over the filled tables:
// the heads by node into hd[0 .. n-1], every lane writing the same values.
// Returns false when the walk gives up.
DEV bool kbest_walk(const int* tab, int n, int m, int lo, int single_root, int K, int rank, const int* finb, int* hd,
                    int* stk, int lane) {
  const KBest T = kbest_tables(const_cast<int*>(tab), m, K);
  for (int i = lane; i < n; i += 64) hd[i] = -1;
  __builtin_amdgcn_wave_barrier();
  int sp = 0;
  // kinds: 0 CR, 1 CL, 2 BS under the arc s -> t, 3 BS under the arc t -> s
#define KBEST_PUSH(kind_, rank_, s_, t_)                                      \
  do {                                                                        \
    if ((s_) < (t_)) {                                                        \
      if (sp >= KBEST_STACK) return false;                                    \
      stk[sp++] = ((kind_) << 20) | ((rank_) << 16) | ((s_) << 8) | (t_);     \
    }                                                                         \
  } while (0)
  if (single_root) {
    const int bp = finb[rank], p = bp >> 8;
    if (p < 0 || p >= m) return false;
    hd[lo + p] = 0;
    KBEST_PUSH(1, (bp >> 4) & 15, 0, p);
    KBEST_PUSH(0, bp & 15, p, m - 1);
  } else {
    KBEST_PUSH(0, rank, 0, m - 1);
  }
  for (int budget = 2 * m; sp > 0; --budget) {
    if (budget <= 0) return false;  // (a derivation has at most 2 m - 1 items)
    const int item = stk[--sp];
    const int kind = item >> 20, r = (item >> 16) & 15, s = (item >> 8) & 255, t = item & 255, L = t - s;
    if (r >= K) return false;
    const int x = r * T.tri + proj_off(L, m) + s;
    const int bp = kind == 0 ? T.crb[x] : kind == 1 ? T.clb[x] : T.bsb[x];
    const int k = bp >> 8, i = (bp >> 4) & 15, j = bp & 15;
    if (k < 0 || k >= L) return false;
    if (kind == 0) {
      KBEST_PUSH(2, i, s, s + k + 1);
      KBEST_PUSH(0, j, s + k + 1, t);
    } else if (kind == 1) {
      KBEST_PUSH(1, i, s, s + k);
      KBEST_PUSH(3, j, s + k, t);
    } else {
      if (kind == 2) hd[lo + t] = lo + s;
      else hd[lo + s] = lo + t;
      KBEST_PUSH(0, i, s, s + k);
      KBEST_PUSH(1, j, s + k + 1, t);
    }
  }
#undef KBEST_PUSH
  __builtin_amdgcn_wave_barrier();
  return true;
}

// scores [b][v][o], n_nodes [b], heads [b][K][v], totals [b][K], count / status
// [b]; ws: ws_stride ints per graph for the graphs that do not fit the LDS.
// grid = b, block = 256.  (A template: its code is emitted after every kernel
// that was there before it, so those keep their places in the code object.)
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_projective_kbest(const int* __restrict__ scores, int o,
                                                            const int* __restrict__ n_nodes, int v, int single_root,
                                                            int K, int* __restrict__ heads, int* __restrict__ totals,
                                                            int* __restrict__ count, int* __restrict__ status, int* ws,
                                                            long ws_stride) {
  static_assert(BLOCK == 256, "four waves");
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = tree_node_count(n_nodes[g], v, o);
  const int* __restrict__ S = scores + (long)g * v * o;
  int* __restrict__ H = heads + (long)g * K * v;
  __shared__ int tab[KBEST_TAB_INTS];
  __shared__ int stk[4][KBEST_STACK], hd[4][TREE_MAXV], finv[KBEST_MAX], finb[KBEST_MAX], wmax[4], flag;

  int st = n < 2 ? 0 : 1;
  if (st) {  // the range rule: S * (n - 1) < 2^30 keeps every total in int32
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
    if ((long long)mx * (n - 1) >= (1LL << 30)) st = 2;
  }
  int cnt = 0;
  if (st == 1) {
    const int lo = single_root ? 1 : 0, m = n - lo;
    int* const T = kbest_in_lds(n, K) ? tab : ws + (long)g * ws_stride;
    if (tid == 0) flag = 0;
    if (kbest_in_lds(n, K)) kbest_fill(tab, S, o, m, lo, single_root, K, finv, finb, tid);
    else kbest_fill(ws + (long)g * ws_stride, S, o, m, lo, single_root, K, finv, finb, tid);
    for (int r = 0; r < K; ++r) cnt += finv[r] != PROJ_NEG;
    // the ranks, a wave each
    for (int r = wave; r < cnt; r += 4) {
      bool ok = kbest_walk(T, n, m, lo, single_root, K, r, finb, hd[wave], stk[wave], lane);
      for (int i = lane; i < v; i += 64) {
        const bool word = ok && i >= 1 && i < n;
        const int h = word ? hd[wave][i] : -1;
        if (word && (h < 0 || h >= n)) ok = false;
        H[(long)r * v + i] = h;
      }
      if (!ok) flag = 1;
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    if (flag || cnt == 0) st = 2, cnt = 0;
  }
  // the absent ranks (every rank of a graph without a list), then the graph's record
  for (long x = (long)cnt * v + tid; x < (long)K * v; x += 256) H[x] = -1;
  if (tid < K) totals[(long)g * K + tid] = tid < cnt ? finv[tid] : TREE_FORBIDDEN;
  if (tid == 0) {
    count[g] = cnt;
    status[g] = st;
  }
}
