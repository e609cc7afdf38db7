// k_tree_loss.h -- the two small kernels either side of the arc-marginal kernels
// (k_lapl.h, k_marg.h) in ggnn_tree_loss, the tree-structured training loss
// (Koo et al. 2007): the negative log-likelihood of the gold tree under the
// distribution over dependency trees that the head probabilities define,
//   L = -sum_d ln p[d][gold_d] + ln Z,   dL/dz[d][k] = marg[d][k] - y[d][k]
// (z the head logits).  The cross-entropy term and its gradient are the heads'
// own (k_head.h); this file adds what is new:
//
// k_tree_loss_gold: whether a graph's gold heads are a tree of the chosen
//   family over the allowed arcs, i.e. whether the gold tree has a probability
//   under the distribution at all.  n_eff[g] = n for such a graph and 0
//   otherwise; the marginal kernel that follows leaves a graph with n_eff = 0
//   alone (marg = a copy of the probabilities, status 0), which is the plain
//   cross-entropy for that graph.  Host form: evaluation.py gold_tree_ok.
//   One workgroup of 256 threads per graph.  Phase 1: one wave per gold row
//   (rows wave, wave + 4, ...), lane l on columns l + 64k, the next row's loads
//   issued before the current row is reduced (the kernel is latency-bound: b
//   workgroups, a few tens of KB each); a row's ones are counted and its first
//   one found by ballots, the head goes to LDS.  Phase 2: one thread per word:
//   its arc's potential, its head chain (at most n steps) and, for the
//   projective family, its arc against every other arc.  No atomics; the
//   graph's verdict is an integer sum of the four waves' counts in LDS.
//
// k_tree_loss_fold: used[g] = (status[g] == 1) and loss[0] += (sum over the
//   used graphs of logz[g]) / target_num.  One wave: lane-strided partial sums
//   in double, one butterfly: a fixed order, the same bytes from launch to
//   launch.
#pragma once
#include "ggnn_common.h"
#include "k_decode.h"
#include "k_marg.h"
#include "k_tree.h"

static_assert(TREE_MAXV <= 256, "k_tree_loss_gold: one thread per word");

// gold [b][v][o] (the head's 0/1 targets), P [b][v][o] (the head probabilities),
// n_nodes [b]; n_eff [b] out.  grid = b, block = 256.  NI * 64 >= o.
template <int NI>
__global__ void __launch_bounds__(256) k_tree_loss_gold(const float* __restrict__ gold, const float* __restrict__ P,
                                                        int o, const int* __restrict__ n_nodes, int v, int family,
                                                        int single_root, int* __restrict__ n_eff) {
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = tree_node_count(n_nodes[g], v, o);
  const long base = (long)g * v;
  __shared__ int s_head[TREE_MAXV];
  __shared__ int s_part[4][2];
  // phase 1: every row of the graph (the rows outside 1..n-1 must be all zero)
  int rows_ok = 1;
  float cur[NI], nxt[NI];
  if (wave < v) decode_load<NI>(gold + (base + wave) * o, o, lane, cur);
  for (int i = wave; i < v; i += 4) {
    if (i + 4 < v) decode_load<NI>(gold + (base + i + 4) * o, o, lane, nxt);
    int ones = 0, idx = -1;
    bool other = false;
#pragma unroll
    for (int k = NI - 1; k >= 0; --k) {
      const int j = lane + 64 * k;
      const unsigned long long hit = __ballot(j < o && cur[k] == 1.0f);
      other |= j < o && !(cur[k] == 0.f || cur[k] == 1.0f);  // (a NaN is neither)
      ones += __popcll(hit);
      if (hit) idx = 64 * k + __ffsll((long long)hit) - 1;
    }
    const bool word = i >= 1 && i < n;
    bool ok = __any(other) == 0 && ones == (word ? 1 : 0);
    if (word && ok) ok = idx < n && idx != i;
    if (!ok) rows_ok = 0;
    if (lane == 0 && i < TREE_MAXV) s_head[i] = (word && ok) ? idx : 0;
#pragma unroll
    for (int k = 0; k < NI; ++k) cur[k] = nxt[k];
  }
  if (lane == 0) s_part[wave][0] = rows_ok;
  __syncthreads();
  // (the same answer in every thread: the whole workgroup leaves together)
  if (n < 2 || !(s_part[0][0] & s_part[1][0] & s_part[2][0] & s_part[3][0])) {
    if (tid == 0) n_eff[g] = 0;
    return;
  }
  __syncthreads();  // s_part is rewritten below
  // phase 2: word tid; every head is in 0..n-1 and is not the word itself
  const bool word = tid >= 1 && tid < n;
  bool bad = false, root = false;
  if (word) {
    const int h = s_head[tid];
    root = h == 0;
    bad = !marg_allowed(P[(base + tid) * o + h]);
    int x = tid;
    for (int s = 0; s < n && x != 0; ++s) x = s_head[x];
    bad |= x != 0;  // a cycle
    if (family == 1) {
      // (i, head_i) crosses (j, head_j): lo_i < lo_j < hi_i < hi_j, ROOT arcs included
      const int lo = min(tid, h), hi = max(tid, h);
      for (int j = 1; j < n; ++j) {
        const int hj = s_head[j], lj = min(j, hj), uj = max(j, hj);
        bad |= lo < lj && lj < hi && hi < uj;
      }
    }
  }
  const int nbad = __popcll(__ballot(bad)), nroot = __popcll(__ballot(root));
  if (lane == 0) {
    s_part[wave][0] = nbad;
    s_part[wave][1] = nroot;
  }
  __syncthreads();
  if (tid == 0) {
    int tb = 0, tr = 0;
    for (int w = 0; w < 4; ++w) {
      tb += s_part[w][0];
      tr += s_part[w][1];
    }
    n_eff[g] = (tb == 0 && (!single_root || tr == 1)) ? n : 0;
  }
}

// status [b], logz [b]; used [b] out, loss[0] in/out.  target_num: the host
// value, or (tn_dev) read from device memory.  grid = 1, block = 64.
__global__ void __launch_bounds__(64) k_tree_loss_fold(const int* __restrict__ status, const float* __restrict__ logz,
                                                       int b, float target_num, const float* __restrict__ tn_dev,
                                                       int* __restrict__ used, float* __restrict__ loss) {
  const int lane = threadIdx.x;
  double acc = 0.0;
  for (int g = lane; g < b; g += 64) {
    const int u = status[g] == 1;
    used[g] = u;
    if (u) acc += (double)logz[g];  // (logz of a graph that is not used is 0 or -inf: never added)
  }
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
  if (lane == 0) {
    const float tn = tn_dev ? tn_dev[0] : target_num;
    loss[0] += (float)(acc / (double)tn);
  }
}
