// k_tree.h -- tree-constrained decoding on the device (btb task): a post-pass
// on k_heads_decode's pred that leaves a graph alone when its arg-max heads
// already are a dependency tree and otherwise replaces them with a maximum
// spanning arborescence of the integer head scores (Chu-Liu/Edmonds).  Host
// form: evaluation.py tree_decode_arrays (the same formulation, step by step).
//
// Graph g, n = its node count, word i in 1..n-1 takes head j in 0..n-1:
//   key(i, j) = scores[i][j] - (single_root && j == 0 ? 2^42 : 0)   (int64)
// so one ROOT child fewer beats any difference of two trees' totals
// (< 2 * 255 * 2^31 < 2^42): with single_root the optimum has one ROOT child
// whenever a single-rooted tree exists, and the result is checked for it.
//
// The contraction never touches the n x n scores.  Every word carries the live
// node of the contraction forest it belongs to (label) and an offset; the
// adjusted score of arc (i, j) is key(i, j) - off[i].  A round
//   A  finds every word's best arc from outside its node (a wave per row, lane
//      l owns columns l + 64k: the maximum by a butterfly, its first column by
//      ballots, as decode_first_max) -- only for words whose best arc's source
//      has joined their own node in the last contraction,
//   B  gives every new node the best of its words' arcs (first word on ties),
//   C  follows the nodes' arcs by pointer jumping: ceil(log2 n) doublings take
//      every node to ROOT or onto a cycle and gather the smallest node id of
//      the 2^K-step path, which on a cycle is the cycle's smallest member,
//   D  contracts ALL cycles: each gets a new forest node (ids in the order of
//      the cycles' smallest members, from ballot prefix sums), the words of
//      its members add their node's best value to their offset and take the
//      new label.
// No cycle: the forest is expanded (one thread; every forest node is entered
// once, from the newest node down: a node that no newer arc entered keeps its
// own best arc, which enters the chain of nodes from its word up to it).
// Adjusted values stay inside [-2^43, 2^31]: every one is a key minus the
// best key of the same node, level by level.
//
// Every loop is bounded by n: at most n rounds (each contracts a cycle of >= 2
// nodes or ends), ceil(log2 n) doublings, fewer than 2n forest nodes, at most
// 2n steps of expansion.  One workgroup of 256 threads per graph, no atomics,
// no inter-workgroup communication; all choices are "first wins" in index
// order, so two launches give the same bytes.
//
// The contraction and the expansion are tree_solve, which reads an arc's score
// through an accessor: k_tree_decode gives it the graph's own scores,
// k_tree_kbest.h the scores under a subproblem's mask.
#pragma once
#include "ggnn_common.h"

#define TREE_MAXV 256                   // GGNN_TREE_MAXV (= the block size: one thread per word)
#define TREE_FORBIDDEN (-2147483647 - 1)  // GGNN_TREE_FORBIDDEN
#define TREE_NONE (-9223372036854775807LL - 1)
#define TREE_ROOT_PENALTY (1LL << 42)

// ---- shared by k_tree.h, k_proj.h and k_marg.h.  The whole workgroup calls
// each helper and none returns past a barrier: a kernel's own early returns
// follow the call, so every thread meets the same barriers.
DEV int tree_node_count(int n_nodes_g, int v, int o) { return max(0, min(n_nodes_g, min(v, min(o, TREE_MAXV)))); }
DEV int tree_doublings(int n) {  // K: 2^K >= n
  int K = 0;
  for (; K < 8 && (1 << K) < n; ++K) {
  }
  return K;
}
// The fast-path check "pred's heads already are a tree".  h: word tid's head
// (-1 for ROOT and past n), ok: an allowed arc (true for ROOT), is_tree: every
// word reaches ROOT, roots: ROOT's children.  tree_pred_arc fills h / ok and
// seeds jp[0..n-1]; tree_pred_follow doubles jp K times and takes the votes.
struct TreePred {
  int h;
  bool ok;
  int is_tree, roots;
};
DEV TreePred tree_pred_arc(const int* __restrict__ pred, const int* __restrict__ S, int o, long base, int n, int* jp,
                           int tid) {
  TreePred t = {-1, tid == 0, 0, 0};
  if (tid > 0 && tid < n) {
    t.h = pred[(base + tid) * 2];
    t.ok = t.h >= 0 && t.h < n && t.h != tid && S[(long)tid * o + t.h] != TREE_FORBIDDEN;
  }
  if (tid < n) jp[tid] = t.ok ? t.h * (tid > 0) : tid;
  return t;
}
DEV void tree_pred_follow(TreePred& t, int n, int K, int* jp, int tid) {
  for (int s = 0; s < K; ++s) {
    __syncthreads();
    const int q = tid < n ? jp[jp[tid]] : 0;
    __syncthreads();
    if (tid < n) jp[tid] = q;
  }
  t.is_tree = __syncthreads_and(tid >= n || (t.ok && jp[tid] == 0));
  t.roots = __syncthreads_count(tid > 0 && tid < n && t.ok && t.h == 0);
}
// las / uas of the repaired graph g, by k_heads_decode's rule (nh: the new
// heads of the words below n); gold and counts both or neither
DEV void tree_recount(const int* __restrict__ gold, int* __restrict__ counts, const int* __restrict__ pred,
                      const int* nh, int n, int v, long base, int g, int tid) {
  if (gold && counts) {
    bool hit_h = false, hit = false;
    if (tid > 0 && tid < v) {
      const long r = (base + tid) * 2;
      const int g_h = gold[r], g_l = gold[r + 1];
      const int p_h = tid < n ? nh[tid] : pred[r], p_l = pred[r + 1];
      hit_h = g_h >= 0 && p_h == g_h;
      hit = hit_h && p_l == g_l;
    }
    const int uas = __syncthreads_count(hit_h), las = __syncthreads_count(hit);
    if (tid == 0) {
      counts[(long)g * DECODE_COUNTS + 1] = las;
      counts[(long)g * DECODE_COUNTS + 2] = uas;
    }
  }
}

// ---- the solver, shared by k_tree_decode and k_tree_kbest.h.  Its state in
// LDS (28 KiB: a kernel declares one __shared__ TreeSolve):
struct TreeSolve {
  // per word
  int label[TREE_MAXV], dirty[TREE_MAXV], wsrc[TREE_MAXV], nh[TREE_MAXV];
  long long off[TREE_MAXV], wval[TREE_MAXV];
  // per forest node (words 0..n-1, contracted cycles n..2n-3)
  int tpar[2 * TREE_MAXV], in_u[2 * TREE_MAXV], in_i[2 * TREE_MAXV], jp[2 * TREE_MAXV], jm[2 * TREE_MAXV],
      oncyc[2 * TREE_MAXV], newid[2 * TREE_MAXV], entered[2 * TREE_MAXV];
  long long bestv[2 * TREE_MAXV];
  int wcnt[8];
};
// an arc's score as the solver reads it: score(i, j) for word i and head j
// below n, TREE_FORBIDDEN = no such arc.  The graph's own scores:
struct TreePlainScores {
  const int* __restrict__ S;
  int o;
  DEV int operator()(int i, int j) const { return S[(long)i * o + j]; }
};

// Rounds A-D and the expansion on the graph whose arcs `score` gives (n >= 2
// nodes, K = tree_doublings(n)).  Called by the whole workgroup of 256 threads
// with the same arguments; true: sh.nh[1 .. n-1] hold the heads of a maximum
// arborescence (with single_root: of one ROOT child), false: no such tree
// exists.  The answer is the same in every thread, and the true return follows
// a barrier after the last write of sh.nh.
template <class Score>
DEV bool tree_solve(TreeSolve& sh, const Score& score, int n, int K, int single_root, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  int *const label = sh.label, *const dirty = sh.dirty, *const wsrc = sh.wsrc, *const nh = sh.nh;
  long long *const off = sh.off, *const wval = sh.wval, *const bestv = sh.bestv;
  int *const tpar = sh.tpar, *const in_u = sh.in_u, *const in_i = sh.in_i, *const jp = sh.jp, *const jm = sh.jm,
             *const oncyc = sh.oncyc, *const newid = sh.newid, *const entered = sh.entered, *const wcnt = sh.wcnt;

  // ---- Chu-Liu/Edmonds
  for (int x = tid; x < 2 * TREE_MAXV; x += 256) tpar[x] = -1;
  label[tid] = tid;
  off[tid] = 0;
  dirty[tid] = 1;
  int nid = n, first_new = 1;
  bool done = false;
  __syncthreads();
  for (int round = 0; round < n; ++round) {
    // A: the best arc into every word whose node changed
    for (int i = 1 + wave; i < n; i += 4) {
      if (!dirty[i]) continue;
      const int li = label[i];
      long long val[4], best = TREE_NONE;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int j = lane + 64 * k;
        val[k] = TREE_NONE;
        if (j < n) {
          const int s = score(i, j);
          if (s != TREE_FORBIDDEN && label[j] != li)
            val[k] = (long long)s - ((single_root && j == 0) ? TREE_ROOT_PENALTY : 0LL);
        }
        best = val[k] > best ? val[k] : best;
      }
      for (int m = 32; m >= 1; m >>= 1) {
        const long long ob = __shfl_xor(best, m);
        best = ob > best ? ob : best;
      }
      int idx = -1;
#pragma unroll
      for (int k = 3; k >= 0; --k) {
        const unsigned long long hit = __ballot(val[k] != TREE_NONE && val[k] == best);
        if (hit) idx = 64 * k + __ffsll((long long)hit) - 1;
      }
      if (lane == 0) {
        wsrc[i] = idx;
        wval[i] = idx >= 0 ? best - off[i] : TREE_NONE;
      }
    }
    __syncthreads();
    // B: the best arc into every new node
    bool none = false;
    for (int x = tid; x < nid; x += 256) {
      if (x < first_new) continue;
      long long bv = TREE_NONE;
      int bi = -1;
      for (int i = 1; i < n; ++i)
        if (label[i] == x && wsrc[i] >= 0 && wval[i] > bv) {
          bv = wval[i];
          bi = i;
        }
      if (bi < 0) {
        none = true;
      } else {
        bestv[x] = bv;
        in_i[x] = bi;
        in_u[x] = wsrc[bi];
      }
    }
    if (__syncthreads_or(none)) return false;  // a node nothing may enter: no tree exists
    // C: follow the live nodes' arcs; node 0 (ROOT) is its own parent
    bool livex[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int x = tid + 256 * s;
      livex[s] = x > 0 && x < nid && tpar[x] < 0;
      jp[x] = livex[s] ? label[in_u[x]] : 0;
      jm[x] = x;
      oncyc[x] = 0;
    }
    for (int step = 0; step < K; ++step) {
      __syncthreads();
      int q[2], mm[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int x = tid + 256 * s, p = jp[x];
        q[s] = jp[p];
        mm[s] = min(jm[x], jm[p]);
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        jp[tid + 256 * s] = q[s];
        jm[tid + 256 * s] = mm[s];
      }
    }
    __syncthreads();
    // (after 2^K >= n steps a node stands on ROOT or on a cycle, and the live
    // nodes of a cycle map onto all of it: every writer stores the same 1)
#pragma unroll
    for (int s = 0; s < 2; ++s)
      if (livex[s] && jp[tid + 256 * s] != 0) oncyc[jp[tid + 256 * s]] = 1;
    __syncthreads();
    bool lead[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int x = tid + 256 * s;
      lead[s] = livex[s] && oncyc[x] && jm[x] == x;
    }
    if (!__syncthreads_or(lead[0] || lead[1])) {
      done = true;
      break;
    }
    // D: one new forest node per cycle, in the order of the cycles' leaders
    int inwave[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const unsigned long long mask = __ballot(lead[s]);
      inwave[s] = __popcll(mask & ((1ULL << lane) - 1ULL));
      if (lane == 0) wcnt[4 * s + wave] = __popcll(mask);
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      int before = 0;
      for (int q = 0; q < 4 * s + wave; ++q) before += wcnt[q];
      if (lead[s]) newid[tid + 256 * s] = nid + before + inwave[s];
    }
    for (int q = 0; q < 8; ++q) total += wcnt[q];
    if (nid + total > 2 * n) return false;  // (cannot happen: every cycle merges >= 2 of < n live nodes)
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int x = tid + 256 * s;
      if (livex[s] && oncyc[x]) tpar[x] = newid[jm[x]];
    }
    const bool word = tid > 0 && tid < n;
    int moved = 0;
    if (word) {
      const int lx = label[tid];
      moved = oncyc[lx];
      if (moved) {
        off[tid] += bestv[lx];
        if (wsrc[tid] >= 0) wval[tid] -= bestv[lx];
        label[tid] = newid[jm[lx]];
      }
    }
    first_new = nid;
    nid += total;
    __syncthreads();
    // a moved word keeps its best arc (now lower by its old node's best value)
    // unless the arc's source joined the same node: only then is its row
    // scanned again (the arc was the first maximum of a superset of columns)
    if (word) dirty[tid] = moved && wsrc[tid] >= 0 && label[wsrc[tid]] == label[tid];
    __syncthreads();
  }
  if (!done) return false;  // (cannot happen: n rounds contract n - 1 cycles at most)

  // ---- expansion of the contraction forest, newest node first
  for (int x = tid; x < 2 * TREE_MAXV; x += 256) entered[x] = 0;
  nh[tid] = -1;
  __syncthreads();
  if (tid == 0) {
    int budget = 2 * n;  // every node is entered once
    for (int x = nid - 1; x >= 1; --x) {
      if (entered[x]) continue;
      const int i = in_i[x];
      nh[i] = in_u[x];
      for (int y = i; y != x && y >= 0 && budget > 0; --budget) {
        entered[y] = 1;
        y = tpar[y];
      }
    }
  }
  __syncthreads();
  {
    const bool word = tid > 0 && tid < n;
    const int hole = __syncthreads_or(word && (nh[tid] < 0 || nh[tid] >= n));
    const int roots = __syncthreads_count(word && nh[tid] == 0);
    if (hole || (single_root && roots != 1)) return false;  // only trees with several ROOT children exist
  }
  return true;
}

// scores [b][v][o], n_nodes [b], pred [b][v][2] in/out, gold [b][v][2] and
// counts [b][DECODE_COUNTS] both or neither, status [b].  grid = b, block = 256.
__global__ void __launch_bounds__(256) k_tree_decode(const int* __restrict__ scores, int o,
                                                     const int* __restrict__ n_nodes, int v, int single_root,
                                                     int* __restrict__ pred, const int* __restrict__ gold,
                                                     int* __restrict__ counts, int* __restrict__ status) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n = tree_node_count(n_nodes[g], v, o);
  const long base = (long)g * v;
  const int* __restrict__ S = scores + base * o;
  if (n < 2) {
    if (tid == 0) status[g] = 0;
    return;
  }
  const int K = tree_doublings(n);
  __shared__ TreeSolve sh;

  // ---- the fast path: pred's heads already are a tree
  TreePred t = tree_pred_arc(pred, S, o, base, n, sh.jp, tid);
  tree_pred_follow(t, n, K, sh.jp, tid);
  if (t.is_tree && (!single_root || t.roots == 1)) {
    if (tid == 0) status[g] = 0;
    return;
  }

  const TreePlainScores score = {S, o};
  if (!tree_solve(sh, score, n, K, single_root, tid)) {
    if (tid == 0) status[g] = 2;
    return;
  }
  if (tid > 0 && tid < n) pred[(base + tid) * 2] = sh.nh[tid];
  if (tid == 0) status[g] = 1;
  tree_recount(gold, counts, pred, sh.nh, n, v, base, g, tid);
}
