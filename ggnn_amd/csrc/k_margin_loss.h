// k_margin_loss.h -- the three small kernels either side of the family's
// decoder (k_tree.h, k_proj.h) in ggnn_margin_loss, the max-margin training
// loss: the structured hinge over cost-augmented decoding,
//   T* = argmax over the family's trees T of sum_d s[d][T_d] + C [T_d != y_d],
//   l  = sum over the words with T*_d != y_d of ln p[d][T*_d] - ln p[d][y_d] + c,
//   L  = max(0, l),   dL/dz[d][k] = onehot(T*)[d][k] - y[d][k] where l > 0, else 0
// (z the head logits, p their softmax, y the gold heads, s the integers of
// tree_scores, C = rint(c 2^k / ln 2)).  The launch order: k_tree_loss_gold
// (k_tree_loss.h: n_eff), k_margin_scores, the decoder on (s', n_eff) with
// every head of pred at -1 so that it always solves, k_margin_fold,
// k_margin_sum.  Host form: evaluation.py margin_loss_arrays.
//
// k_margin_scores: s' int32 [b][v][o], the gold heads int32 [b][v] and pred
//   int32 [b][v][2] = -1 of every eligible graph (n_eff >= 2; the decoder and
//   the fold read nothing of any other graph).  One workgroup of 256 threads
//   per graph, one wave per row (rows wave, wave + 4, ...), lane l on columns
//   l + 64k, the next row's loads issued before the current row is worked on,
//   as in k_tree_loss_gold phase 1.  log2 in double on the float32 p, then
//   rint: the integers of evaluation.tree_scores.
//
// k_margin_fold: one workgroup per graph.  used = eligible and status 1; one
//   thread per word for l (double), the Hamming distance and sum_d ln
//   p[d][y_d], reduced in a fixed order (a butterfly per wave, the four waves'
//   sums added in wave order); then the graph's [v][o] block of marg: onehot(T*)
//   where used and l > 0, the gold block where used and l <= 0, the
//   probabilities' bytes otherwise.
//
// k_margin_sum: loss[0] += (sum over the used graphs of term[g]) / target_num,
//   term[g] = max(0, l) + sum_d ln p[d][y_d] (the second part cancels the
//   cross-entropy the heads' forward has put into the loss).  One wave, lane-
//   strided doubles, one butterfly: k_tree_loss_fold's order.
#pragma once
#include "ggnn_common.h"
#include "k_decode.h"
#include "k_marg.h"
#include "k_tree.h"

static_assert(TREE_MAXV <= 256, "k_margin_fold: one thread per word");

// gold [b][v][o], P [b][v][o], n_eff [b]; S [b][v][o], goldh [b][v], pred
// [b][v][2] out.  scale = 2^k, floor_q = -150 * 2^k, C: the cost in score
// units.  grid = b, block = 256.  NI * 64 >= o.
template <int NI>
__global__ void __launch_bounds__(256) k_margin_scores(const float* __restrict__ gold, const float* __restrict__ P,
                                                       int o, const int* __restrict__ n_eff, int v, double scale,
                                                       double floor_q, int C, int* __restrict__ S,
                                                       int* __restrict__ goldh, int* __restrict__ pred) {
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(n_eff[g], min(v, TREE_MAXV));
  if (n < 2) return;  // (the same answer in every thread)
  const long base = (long)g * v;
  float yc[NI], pc[NI], yn[NI], pn[NI];
  if (wave < v) {
    decode_load<NI>(gold + (base + wave) * o, o, lane, yc);
    decode_load<NI>(P + (base + wave) * o, o, lane, pc);
  }
  for (int i = wave; i < v; i += 4) {
    if (i + 4 < v) {
      decode_load<NI>(gold + (base + i + 4) * o, o, lane, yn);
      decode_load<NI>(P + (base + i + 4) * o, o, lane, pn);
    }
    const bool word = i >= 1 && i < n;
    int y = -1;
#pragma unroll
    for (int k = NI - 1; k >= 0; --k) {
      const unsigned long long hit = __ballot(lane + 64 * k < o && yc[k] == 1.0f);
      if (hit) y = 64 * k + __ffsll((long long)hit) - 1;
    }
    if (!word) y = -1;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      const int j = lane + 64 * k;
      if (j < o) {
        int s = TREE_FORBIDDEN;
        if (word && j < n && j != i && marg_allowed(pc[k])) {
          const double q = fmax(rint(log2((double)pc[k]) * scale), floor_q);
          s = (int)q + (j != y ? C : 0);
        }
        S[(base + i) * o + j] = s;
      }
    }
    if (lane == 0) {
      goldh[base + i] = y;
      pred[(base + i) * 2] = -1;
      pred[(base + i) * 2 + 1] = -1;
    }
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      yc[k] = yn[k];
      pc[k] = pn[k];
    }
  }
}

// P, gold [b][v][o], n_eff [b], goldh [b][v], pred [b][v][2] (the decoder's),
// status [b]; marg [b][v][o], heads [b][v], value [b], hamming [b], used [b],
// term [b] (double) out.  grid = b, block = 256.
__global__ void __launch_bounds__(256) k_margin_fold(const float* __restrict__ P, const float* __restrict__ gold, int o,
                                                     const int* __restrict__ n_eff, int v,
                                                     const int* __restrict__ goldh, const int* __restrict__ pred,
                                                     const int* __restrict__ status, double cost,
                                                     float* __restrict__ marg, int* __restrict__ heads,
                                                     float* __restrict__ value, int* __restrict__ hamming,
                                                     int* __restrict__ used, double* __restrict__ term) {
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(n_eff[g], min(v, TREE_MAXV));
  const bool u = n >= 2 && status[g] == 1;
  const long base = (long)g * v;
  __shared__ int s_t[TREE_MAXV];
  __shared__ double s_l[4], s_y[4];
  __shared__ int s_h[4];
  // word tid: its part of l, of the Hamming distance and of sum_d ln p[d][y_d]
  int t = -1;
  double l = 0.0, ly = 0.0;
  int wrong = 0;
  if (u && tid >= 1 && tid < n) {
    t = pred[(base + tid) * 2];
    const int y = goldh[base + tid];
    // (status 1: t is an allowed arc; eligible: so is y; a head outside the row would be a fault of the decoder)
    if (t >= 0 && t < n && y >= 0 && y < n) {
      ly = log((double)P[(base + tid) * o + y]);
      if (t != y) {
        l = log((double)P[(base + tid) * o + t]) - ly + cost;
        wrong = 1;
      }
    } else {
      t = -1;
    }
  }
  for (int i = tid; i < v; i += 256) heads[base + i] = i < TREE_MAXV ? t : -1;  // (v <= TREE_MAXV: i == tid)
  if (tid < TREE_MAXV) s_t[tid] = t;
  for (int m = 32; m >= 1; m >>= 1) {
    l += __shfl_xor(l, m);
    ly += __shfl_xor(ly, m);
  }
  const int nw = __popcll(__ballot(wrong != 0));
  if (lane == 0) {
    s_l[wave] = l;
    s_y[wave] = ly;
    s_h[wave] = nw;
  }
  __syncthreads();
  const double lt = ((s_l[0] + s_l[1]) + s_l[2]) + s_l[3];
  const bool active = u && lt > 0.0;
  if (tid == 0) {
    used[g] = u ? 1 : 0;
    value[g] = active ? (float)lt : 0.f;
    hamming[g] = u ? s_h[0] + s_h[1] + s_h[2] + s_h[3] : 0;
    term[g] = u ? (active ? lt : 0.0) + (((s_y[0] + s_y[1]) + s_y[2]) + s_y[3]) : 0.0;
  }
  // the graph's block of marg
  const unsigned* __restrict__ Pb = (const unsigned*)P;
  const unsigned* __restrict__ Yb = (const unsigned*)gold;
  unsigned* __restrict__ Mb = (unsigned*)marg;
  for (int i = wave; i < v; i += 4) {
    const long row = (base + i) * o;
    const int ti = (active && i < TREE_MAXV) ? s_t[i] : -1;
    for (int j = lane; j < o; j += 64) {
      unsigned x;
      if (active) x = (j == ti) ? 0x3F800000u : 0u;  // 1.0f / 0.0f
      else if (u) x = Yb[row + j];
      else x = Pb[row + j];
      Mb[row + j] = x;
    }
  }
}

// used [b], term [b]; loss[0] in/out.  target_num: the host value, or (tn_dev)
// read from device memory.  grid = 1, block = 64.
__global__ void __launch_bounds__(64) k_margin_sum(const int* __restrict__ used, const double* __restrict__ term, int b,
                                                   float target_num, const float* __restrict__ tn_dev,
                                                   float* __restrict__ loss) {
  const int lane = threadIdx.x;
  double acc = 0.0;
  for (int g = lane; g < b; g += 64)
    if (used[g]) acc += term[g];
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
  if (lane == 0) {
    const float tn = tn_dev ? tn_dev[0] : target_num;
    loss[0] += (float)(acc / (double)tn);
  }
}
