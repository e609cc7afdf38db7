// k_decode.h -- on-device decoding of the two heads' probabilities (btb task):
// the predicted head / label of every node and the per-graph LAS / UAS counts,
// with the semantics of the host scorer (evaluation.py: results_reshaped_btb +
// _first_max, i.e. chem_tensorflow_dense.py:1054-1079 and :106-131):
//   node i of graph g (n = its node count, rows 1..v-1 are scored)
//     head   first maximum over the o columns of  p[j] * (j < n ? 1 : 0)
//     label  first maximum over the oe columns of p[j]
//     both skipped (-1) when i >= n, the maximum is 0 or the masked row holds a
//     NaN (numpy's max propagates it and equals nothing)
//     gold   first column equal to 1.0f (no such column: skipped)
//   regular[g] = the four lists (two without gold) skip the same nodes and no
//     input of a row i < n is NaN or +-inf (masked columns included: inf * 0
//     is NaN on the host); otherwise the host's list path must score the graph
// One workgroup of 256 threads per graph, one wave per node row (rows
// 1 + wave, 5 + wave, ...), lane l owns columns l + 64k; a wave reduces with
// "larger value wins, equal values: smaller column wins" (the maximum by a
// butterfly, its smallest column by ballots).  No atomics, no
// inter-workgroup communication: the graph's counters are integer sums of the
// four waves' partials, added in wave order in LDS -- the same bytes run to run.
#pragma once
#include "ggnn_common.h"

#define DECODE_COUNTS 5  // n_kept, las, uas, lab, regular (GGNN_DECODE_COUNTS)

struct DecodeRow {
  int idx;   // first maximum's column, -1 = skipped
  bool bad;  // a NaN or +-inf among the row's inputs
};

// a row's columns lane + 64k in registers (NI * 64 >= w; 0 past the row's end)
template <int NI>
DEV void decode_load(const float* __restrict__ row, int w, int lane, float (&x)[NI]) {
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    const int j = lane + 64 * k;
    x[k] = j < w ? row[j] : 0.f;
  }
}

// first maximum of x[j] * (j < n ? 1 : 0) over j < w (the whole wave calls it):
// the wave's maximum by a butterfly, then its first column from one ballot per
// 64-column chunk, chunks ascending (6 cross-lane exchanges instead of the 18 of
// a (value, column) butterfly: the row's dependent chain is what the kernel waits on)
template <int NI>
DEV DecodeRow decode_first_max(const float (&x)[NI], int w, int n, int lane) {
  float val[NI];
  float best = -INFINITY;
  bool bad = false, nan = false;
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    const int j = lane + 64 * k;
    val[k] = j < n ? x[k] : x[k] * 0.f;
    if (j < w) {
      bad |= !(fabsf(x[k]) <= 3.402823466e38f);
      nan |= val[k] != val[k];
      best = val[k] > best ? val[k] : best;
    }
  }
  for (int m = 32; m >= 1; m >>= 1) {
    const float ob = __shfl_xor(best, m);
    best = ob > best ? ob : best;
  }
  int idx = -1;
#pragma unroll
  for (int k = NI - 1; k >= 0; --k) {
    const int j = lane + 64 * k;
    const unsigned long long hit = __ballot(j < w && val[k] == best);
    if (hit) idx = 64 * k + __ffsll((long long)hit) - 1;
  }
  DecodeRow r;
  r.bad = __any(bad) != 0;
  r.idx = (__any(nan) != 0 || best == 0.f) ? -1 : idx;
  return r;
}

// first column of x[0..w) equal to 1.0f, -1 if none (the whole wave calls it)
template <int NI>
DEV int decode_first_one(const float (&x)[NI], int w, int lane) {
  int idx = -1;
#pragma unroll
  for (int k = NI - 1; k >= 0; --k) {
    const int j = lane + 64 * k;
    const unsigned long long hit = __ballot(j < w && x[k] == 1.0f);
    if (hit) idx = 64 * k + __ffsll((long long)hit) - 1;
  }
  return idx;
}

// probs_head [b][v][o], probs_label [b][v][oe], gold_head / gold_label the same
// shapes or both NULL, n_nodes [b]; pred / gold [b][v][2] (head, label), counts
// [b][DECODE_COUNTS].  grid = b, block = 256.  NI: 64-column chunks per lane,
// NI * 64 >= max(o, oe).  A row's four inputs are loaded before the first
// reduction: one memory round trip per row instead of four (the kernel is
// latency-bound: b workgroups, a few KB each).
template <int NI>
__global__ void __launch_bounds__(256) k_heads_decode(const float* __restrict__ ph, int o,
                                                      const float* __restrict__ pl, int oe,
                                                      const float* __restrict__ gh, const float* __restrict__ gl,
                                                      const int* __restrict__ n_nodes, int v, int* __restrict__ pred,
                                                      int* __restrict__ gold, int* __restrict__ counts) {
  const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = max(0, min(n_nodes[g], min(v, o)));
  const long base = (long)g * v;
  int kept = 0, las = 0, uas = 0, lab = 0, regular = 1;
  if (threadIdx.x == 0) {  // row 0 (ROOT) is never scored
    pred[base * 2] = pred[base * 2 + 1] = -1;
    if (gold) gold[base * 2] = gold[base * 2 + 1] = -1;
  }
  for (int i = 1 + wave; i < v; i += 4) {
    const long r = base + i;
    float xh[NI], xl[NI], yh[NI], yl[NI];
    if (i < n) {
      decode_load<NI>(ph + r * o, o, lane, xh);
      decode_load<NI>(pl + r * oe, oe, lane, xl);
    }
    if (gh) {
      decode_load<NI>(gh + r * o, o, lane, yh);
      decode_load<NI>(gl + r * oe, oe, lane, yl);
    }
    int p_h = -1, p_l = -1, g_h = -1, g_l = -1;
    if (i < n) {
      const DecodeRow a = decode_first_max<NI>(xh, o, n, lane);
      const DecodeRow c = decode_first_max<NI>(xl, oe, oe, lane);
      p_h = a.idx;
      p_l = c.idx;
      if (a.bad || c.bad) regular = 0;
    }
    if (gh) {
      g_h = decode_first_one<NI>(yh, o, lane);
      g_l = decode_first_one<NI>(yl, oe, lane);
    }
    if (lane == 0) {
      pred[r * 2] = p_h;
      pred[r * 2 + 1] = p_l;
      if (gold) {
        gold[r * 2] = g_h;
        gold[r * 2 + 1] = g_l;
      }
    }
    const bool k = p_h >= 0;
    if ((p_l >= 0) != k) regular = 0;
    if (gh) {
      if ((g_h >= 0) != k || (g_l >= 0) != k) regular = 0;
      if (g_h >= 0) {
        const bool hit_h = p_h == g_h, hit_l = p_l == g_l;
        kept += 1;
        uas += hit_h;
        lab += hit_l;
        las += hit_h && hit_l;
      }
    }
  }
  // (every lane of a wave holds the wave's sums: the row results are wave-uniform)
  __shared__ int part[4][DECODE_COUNTS];
  if (lane == 0) {
    part[wave][0] = kept;
    part[wave][1] = las;
    part[wave][2] = uas;
    part[wave][3] = lab;
    part[wave][4] = regular;
  }
  __syncthreads();
  if (threadIdx.x < DECODE_COUNTS) {
    const int c = threadIdx.x;
    int x = part[0][c];
    for (int w = 1; w < 4; ++w) x = c == 4 ? (x & part[w][c]) : x + part[w][c];
    counts[(long)g * DECODE_COUNTS + c] = x;
  }
}
