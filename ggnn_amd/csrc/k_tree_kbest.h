// k_tree_kbest.h -- the K best dependency trees of the integer head scores
// over ALL dependency trees (arcs may cross), in order, on the device: Lawler's
// partitioning over k_tree.h's Chu-Liu/Edmonds solver.  Host form:
// evaluation.py tree_kbest_arrays.
//
// A SUBPROBLEM is the set of trees that obey a partial head assignment fix[w]
// in {-1, head} and a list of excluded arcs (word, head).  Its best tree is
// the maximum arborescence of the MASKED scores: the row of a fixed word is
// TREE_FORBIDDEN except at column fix[w], every excluded arc is
// TREE_FORBIDDEN; tree_solve reads them through TreeMaskedScores, the n x n
// scores are never copied.  single_root is k_tree.h's 2^42 ROOT penalty and its
// check of the result: a masked problem whose optimum has another number of
// ROOT children holds no single-rooted tree.
//
// Rank 0 is the best tree of the unconstrained problem.  The tree h that
// becomes rank r, with its subproblem's fix and exclusions X, leaves one CHILD
// per word w that fix leaves free, in increasing w: child (r, w) fixes every
// free word w' < w to h[w'] and excludes (w, h[w]) on top of X.  The children
// partition "the subproblem without h": no tree is met twice.  The POOL holds
// every solved child's total; rank r + 1 is the pool's first entry in the
// total order: larger total first, then the smaller parent rank, then the
// smaller word.  As a 64-bit key, larger = earlier:
//   key = total * 2^16 + (15 - parent) * 2^8 + (255 - word)
// A chain of children adds one exclusion per rank: at most K - 1 <= 15.  The
// list ends when the pool is empty; nothing depends on K, so the list for K is
// a prefix of the list for a larger K.
//
// Two kernels alternate on the stream, 2 K - 1 launches, no host
// synchronisation:
//   take(r)   grid b.  r = 0: the range rule and the unconstrained problem.
//             r > 0 (rank r - 1 exists): the pool's first entry (p, w) by a
//             reduction of the keys, child (p, w) solved AGAIN for its heads
//             (they were never stored), the entry marked taken.  Writes
//             heads[g][r], totals[g][r], count, status (r = 0) and rank r's
//             record (fix, exclusions) to the workspace.
//   solve(r)  grid b * (v - 1), workgroup (g, w): leaves at once when rank r
//             does not exist or w >= n; a word fixed in rank r has no child
//             ("none" in the pool); otherwise solves child (r, w) and writes
//             its total, or "none", to pool[g][r][w].
// take(r) reads the pool rows p < r of the words below n only, and only when
// ranks 0 .. r - 1 exist: solve(p) wrote every one of them.
//
// Workspace, int32 per graph: 16 (word 0: the ranks so far) + K * v (the pool)
// + K * (v + 16) (per rank: fix[v], 15 exclusions as word << 16 | head, their
// number) = K (2 v + 16) + 16.  Nothing of size v^2.
//
// One workgroup of 256 threads per problem, LDS 30.2 KiB (TreeSolve + the
// mask: five workgroups fit a CU), no atomics, nothing between the workgroups
// of a launch, every loop bounded by a function of n and K, every tie by index
// order: two calls give the same bytes.
#pragma once
#include "k_proj_kbest.h"
#include "k_tree.h"

#define TKB_HDR 16                          // ints ahead of a graph's pool
#define TKB_REC(v) ((v) + KBEST_MAX)        // ints of a rank's record
#define TKB_STRIDE(v, K) (TKB_HDR + (long)(K) * (v) + (long)(K) * TKB_REC(v))

static_assert(KBEST_MAX == 16 && TREE_MAXV <= 256, "a pool key packs a parent rank below 16 and a word below 256");

// the constraints of one subproblem, in LDS
struct TreeMask {
  int fix[TREE_MAXV];   // the head a word is fixed to, -1 = free
  int hasx[TREE_MAXV];  // the word has an excluded arc
  int ex[KBEST_MAX];    // word << 16 | head, nx of them
  int nx;
};
struct TreeMaskedScores {
  const int* __restrict__ S;
  int o;
  const TreeMask* m;
  DEV int operator()(int i, int j) const {
    const int f = m->fix[i];
    if (f >= 0 && j != f) return TREE_FORBIDDEN;
    int s = S[(long)i * o + j];
    if (m->hasx[i])
      for (int e = 0; e < m->nx; ++e)
        if (m->ex[e] == ((i << 16) | j)) s = TREE_FORBIDDEN;
    return s;
  }
};

// mk = the unconstrained problem.  Whole workgroup; ends in a barrier.
DEV void tkb_mask_clear(TreeMask& mk, int tid) {
  mk.fix[tid] = -1;
  mk.hasx[tid] = 0;
  if (tid == 0) mk.nx = 0;
  __syncthreads();
}
// mk = child (p, w): rec = rank p's record, ph = rank p's heads [v].  Whole
// workgroup; ends in a barrier.
DEV void tkb_mask_child(TreeMask& mk, const int* rec, const int* ph, int v, int n, int w, int tid) {
  int f = -1;
  if (tid >= 1 && tid < n) {
    f = rec[tid];
    if (f < 0 && tid < w) f = ph[tid];
  }
  mk.fix[tid] = f;
  mk.hasx[tid] = 0;
  __syncthreads();
  if (tid == 0) {
    const int nx = max(0, min(rec[v + KBEST_MAX - 1], KBEST_MAX - 2));
    for (int e = 0; e < nx; ++e) {
      const int x = rec[v + e];
      mk.ex[e] = x;
      mk.hasx[(x >> 16) & (TREE_MAXV - 1)] = 1;
    }
    mk.ex[nx] = (w << 16) | ph[w];
    mk.hasx[w] = 1;
    mk.nx = nx + 1;
  }
  __syncthreads();
}
// the sum of the scores of the heads in nh; whole workgroup, the same value in
// every thread
DEV long long tkb_total(const int* __restrict__ S, int o, const int* nh, int n, long long* red, int tid) {
  long long t = (tid >= 1 && tid < n) ? (long long)S[(long)tid * o + nh[tid]] : 0LL;
  for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m);
  __syncthreads();  // (red may still be read from an earlier use)
  if ((tid & 63) == 0) red[tid >> 6] = t;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// scores [b][v][o], n_nodes [b], heads [b][K][v], totals [b][K], count / status
// [b], ws: stride ints per graph.  grid = b, block = 256.  (Templates, as
// k_projective_kbest: their code follows every kernel that was there before.)
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_tree_kbest_take(const int* __restrict__ scores, int o,
                                                           const int* __restrict__ n_nodes, int v, int single_root,
                                                           int K, int r, int* heads, int* __restrict__ totals,
                                                           int* __restrict__ count, int* __restrict__ status, int* ws,
                                                           long stride) {
  static_assert(BLOCK == 256, "one thread per word, four waves");
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = tree_node_count(n_nodes[g], v, o);
  const int* __restrict__ S = scores + (long)g * v * o;
  int* const H = heads + ((long)g * K + r) * v;
  int* const W = ws + (long)g * stride;
  int* const pool = W + TKB_HDR;
  int* const recs = pool + (long)K * v;
  __shared__ TreeSolve sh;
  __shared__ TreeMask mk;
  __shared__ long long red[4];
  __shared__ int wmax[4];

  int st = 0, taken = -1;
  bool have = false;
  if (r == 0) {
    st = n < 2 ? 0 : 1;
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
    if (st == 1) {
      tkb_mask_clear(mk, tid);
      const TreePlainScores score = {S, o};
      have = tree_solve(sh, score, n, tree_doublings(n), single_root, tid);
      if (!have) st = 2;
    }
  } else if (W[0] == r && n >= 2) {  // ranks 0 .. r - 1 exist: the pool's first entry
    long long best = TREE_NONE;
    if (tid >= 1 && tid < n)
      for (int p = 0; p < r; ++p) {
        const int t = pool[(long)p * v + tid];
        if (t == TREE_FORBIDDEN) continue;
        const long long key = (long long)t * 65536 + ((KBEST_MAX - 1 - p) << 8) + (255 - tid);
        best = key > best ? key : best;
      }
    for (int m = 32; m >= 1; m >>= 1) {
      const long long ob = __shfl_xor(best, m);
      best = ob > best ? ob : best;
    }
    if (lane == 0) red[wave] = best;
    __syncthreads();
    for (int q = 0; q < 4; ++q) best = red[q] > best ? red[q] : best;
    if (best != TREE_NONE) {
      const int low = (int)(best & 0xFFFF), p = KBEST_MAX - 1 - (low >> 8), w = 255 - (low & 255);
      tkb_mask_child(mk, recs + (long)p * TKB_REC(v), heads + ((long)g * K + p) * v, v, n, w, tid);
      const TreeMaskedScores score = {S, o, &mk};
      have = tree_solve(sh, score, n, tree_doublings(n), single_root, tid);
      taken = p * v + w;
    }
  }

  if (have) {
    const long long total = tkb_total(S, o, sh.nh, n, red, tid);
    for (int i = tid; i < v; i += BLOCK) H[i] = (i >= 1 && i < n) ? sh.nh[i] : -1;
    int* const rec = recs + (long)r * TKB_REC(v);
    for (int i = tid; i < v; i += BLOCK) rec[i] = mk.fix[i];
    if (tid < KBEST_MAX - 1) rec[v + tid] = tid < mk.nx ? mk.ex[tid] : 0;
    if (tid == 0) {
      rec[v + KBEST_MAX - 1] = mk.nx;
      totals[(long)g * K + r] = (int)total;
      count[g] = r + 1;
      W[0] = r + 1;
      if (taken >= 0) pool[taken] = TREE_FORBIDDEN;
    }
  } else {
    for (int i = tid; i < v; i += BLOCK) H[i] = -1;
    if (tid == 0) {
      totals[(long)g * K + r] = TREE_FORBIDDEN;
      if (r == 0) count[g] = 0, W[0] = 0;
    }
  }
  if (r == 0 && tid == 0) status[g] = st;
}

// heads [b][K][v]: rank r's row is read.  grid = b * (v - 1), block = 256.
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_tree_kbest_solve(const int* __restrict__ scores, int o,
                                                            const int* __restrict__ n_nodes, int v, int single_root,
                                                            int K, int r, const int* __restrict__ heads, int* ws,
                                                            long stride) {
  static_assert(BLOCK == 256, "one thread per word, four waves");
  const int g = blockIdx.x / (v - 1), w = 1 + blockIdx.x % (v - 1), tid = threadIdx.x;
  const int n = tree_node_count(n_nodes[g], v, o);
  int* const W = ws + (long)g * stride;
  if (w >= n || W[0] <= r) return;
  int* const slot = W + TKB_HDR + (long)r * v + w;
  const int* const rec = W + TKB_HDR + (long)K * v + (long)r * TKB_REC(v);
  if (rec[w] >= 0) {  // a fixed word has no child
    if (tid == 0) *slot = TREE_FORBIDDEN;
    return;
  }
  const int* __restrict__ S = scores + (long)g * v * o;
  __shared__ TreeSolve sh;
  __shared__ TreeMask mk;
  __shared__ long long red[4];
  tkb_mask_child(mk, rec, heads + ((long)g * K + r) * v, v, n, w, tid);
  const TreeMaskedScores score = {S, o, &mk};
  const bool have = tree_solve(sh, score, n, tree_doublings(n), single_root, tid);
  long long total = 0;
  if (have) total = tkb_total(S, o, sh.nh, n, red, tid);
  if (tid == 0) *slot = have ? (int)total : TREE_FORBIDDEN;
}
