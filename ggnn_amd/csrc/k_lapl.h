// k_lapl.h -- arc marginals over ALL dependency trees on the device (btb task):
// the matrix-tree theorem (Koo et al. 2007; Smith & Smith 2007; McDonald &
// Satta 2007), the non-projective twin of k_marg.h.  For every graph the
// posterior marginal of every arc "word i takes head j" under the distribution
// over dependency trees (crossing arcs included) whose weight is the product
// of the words' head probabilities, the log of the total weight, and (when
// asked) the integer scores rint(marg * 2^20) whose maximum spanning tree
// (k_tree.h) is the minimum Bayes risk tree.  Host form: evaluation.py
// tree_marginals_arrays (the same formulation, np.linalg for the elimination).
//
// Potentials: p[i][j] of an allowed arc (finite, > 0, 1 <= i < n, j < n, j !=
// i), 0 otherwise.  Every word's row is divided by its own sum c[i] (no
// marginal changes, ln Z gets sum ln c[i] back); the row is first scaled by
// the power of two of its largest entry, which is exact, so a row of fp32
// subnormals loses nothing.  With w(d, h) the normalised potential of word d
// taking word h and r(d) that of d taking ROOT, A is (n-1) x (n-1) over the
// words, m = n - 1:
//   A[h][d] = -w(d, h)  (h != d)
//   multi-root:   A[d][d] = r(d) + sum_h w(d, h)  (= 1 after normalisation)
//                 Z = det A,  B = inverse of A
//                 marg(d takes h) = w(d, h) (B[d][d] - B[d][h]),  marg(d takes ROOT) = r(d) B[d][d]
//   single_root:  A[d][d] = sum_h w(d, h), then the first word's row holds r(.)   (Koo et al.)
//                 marg(d takes h) = [d != first] w(d, h) B[d][d] - [h != first] w(d, h) B[d][h]
//                 marg(d takes ROOT) = r(d) B[d][first]
//
// Whether a tree exists is decided on the ARCS, before any arithmetic (a
// structurally singular A may leave a tiny non-zero pivot after rounding):
// 256-bit rows "node j reaches node i walking head -> dependent", squared
// until paths of n - 1 arcs are covered.  Multi-root: node 0 reaches every
// word; single_root: some word with an allowed ROOT arc reaches every word.
//
// Elimination: in-place Gauss-Jordan inversion with partial pivoting, both
// root modes through the same code (the single-root matrix is not diagonally
// dominant).  In column k the pivot is the largest |A[i][k]| over the rows not
// yet used as a pivot, the smallest row index among equals.  Rows are NOT
// exchanged: row sig[k] serves column k, the result is the inverse of the
// row-permuted matrix in permuted storage,
//   B[i][l] = S[sig[i]][sinv[l]]      (sinv: the inverse of sig)
// and det A = sgn(sig) * the product of the pivots.  ln Z = sum ln |pivot| +
// sum ln c[i], accumulated in double in a fixed order; status 2 when a pivot
// is 0 / not finite, the determinant's sign is not positive or ln Z is not
// finite.
//
// Layout: S row-major with an odd row stride LD = m | 1 dwords.  The rank-1
// update walks S flat, consecutive lanes on consecutive dwords (conflict-free
// reads and writes of S; the pivot row prow[j] consecutive, the multiplier
// col[i] a broadcast); the multiplier column A[.][k] is read once per column
// at stride LD, which being odd spreads it over all banks.  Per column: the
// first m threads (at most four waves, each finding the pivot for itself: one
// wave reduction of a 64-bit key |value| : ~index) stage the scaled pivot row
// and the multiplier column, barrier, every thread updates, barrier.
//
// One workgroup of 1024 threads per graph, two barriers per column, no
// atomics, nothing passes between workgroups, every loop is bounded by a
// function of n, every reduction has a fixed order: two launches give the
// same bytes.
#pragma once
#include <cfloat>

#include "ggnn_common.h"
#include "k_marg.h"
#include "k_tree.h"

#define LAPL_LDS_MAXN 199  // GGNN_LAPL_LDS_MAXN
#define LAPL_THREADS 1024
#define LAPL_WAVES (LAPL_THREADS / 64)
#define LAPL_LD(m) ((m) | 1)  // odd row stride, in dwords
#define LAPL_MAT_FLOATS ((LAPL_LDS_MAXN - 1) * LAPL_LD(LAPL_LDS_MAXN - 1))
#define LAPL_BIT_WORDS (TREE_MAXV / 32)

// what a graph keeps beside its matrix (indexed by word - 1)
struct LaplShared {
  float col[TREE_MAXV];   // the multiplier column of the current step
  float prow[TREE_MAXV];  // the scaled pivot row of the current step
  float pv[TREE_MAXV];    // the pivot record
  float csum[TREE_MAXV];  // c[i] = csum * 2^cexp
  short cexp[TREE_MAXV];
  short sig[TREE_MAXV];   // the row that served column k
  short sinv[TREE_MAXV];  // the column a row served, -1: not yet a pivot row
  int ctl[4];             // pivot row, pivot unusable, determinant positive
  double lnz;
};

// The reachability rows of a graph (see above).  R: 2 * LAPL_BIT_WORDS *
// TREE_MAXV words, word w of node j's row at [w * TREE_MAXV + j].  Returns
// the half of R that holds the finished rows.  Called by the whole workgroup.
DEV const unsigned* lapl_reach(unsigned* R, const float* __restrict__ P, int o, int n, int tid) {
  const int nw = (n + 31) >> 5, half = LAPL_BIT_WORDS * TREE_MAXV;
  for (int x = tid; x < n * nw; x += LAPL_THREADS) {
    const int w = x / n, j = x - w * n;
    unsigned bits = 0;
    const int i1 = min(n, (w + 1) * 32);
    for (int i = max(1, w * 32); i < i1; ++i)
      if (i != j && marg_allowed(P[(long)i * o + j])) bits |= 1u << (i & 31);
    if ((j >> 5) == w) bits |= 1u << (j & 31);
    R[w * TREE_MAXV + j] = bits;
  }
  __syncthreads();
  int cur = 0;
  for (int hops = 1; hops < n; hops <<= 1) {  // one boolean squaring: paths of up to 2 * hops arcs
    const unsigned* A = R + cur * half;
    unsigned* B = R + (cur ^ 1) * half;
    for (int x = tid; x < n * nw; x += LAPL_THREADS) {
      const int w = x / n, j = x - w * n;
      unsigned acc = 0;
      for (int u = 0; u < nw; ++u) {
        unsigned s = A[u * TREE_MAXV + j];
        while (s) {  // (at most 32 rounds)
          const int i = (u << 5) + __ffs((int)s) - 1;
          s &= s - 1;
          acc |= A[w * TREE_MAXV + i];
        }
      }
      B[w * TREE_MAXV + j] = acc;
    }
    __syncthreads();
    cur ^= 1;
  }
  return R + cur * half;
}

// Whether node tid may be the root of every word: node 0 (multi-root) or a word
// with an allowed ROOT arc (single_root) that reaches every word.  A:
// lapl_reach's rows.
DEV bool lapl_root_ok(const unsigned* A, const float* __restrict__ P, int o, int n, int single_root, int tid) {
  const int nw = (n + 31) >> 5;
  bool good = false;
  if (tid < n && (single_root ? (tid >= 1 && marg_allowed(P[(long)tid * o])) : tid == 0)) {
    good = true;
    for (int w = 0; w < nw; ++w) {
      unsigned need = (n - w * 32 >= 32) ? ~0u : ((1u << (n - w * 32)) - 1u);
      if (w == 0) need &= ~1u;  // the words: nodes 1..n-1
      good = good && (A[w * TREE_MAXV + tid] & need) == need;
    }
  }
  return good;
}

// Whether a dependency tree exists over the allowed arcs (see above).  R: as
// lapl_reach's.  Called by the whole workgroup; the same answer in every thread.
DEV bool lapl_has_tree(unsigned* R, const float* __restrict__ P, int o, int n, int single_root, int tid) {
  const unsigned* A = lapl_reach(R, P, o, n, tid);
  return __syncthreads_or(lapl_root_ok(A, P, o, n, single_root, tid)) != 0;
}

// lapl_solve in its pieces (each called by the whole workgroup; S: m *
// LAPL_LD(m) floats, LDS or global).  lapl_build: the row sums and the matrix.
// rho = 0: the matrix of single_root as said above.  rho >= 1 (the sampler,
// k_tree_sample.h): the multi-root matrix of the trees whose one ROOT child is
// word rho: r'(d) = [d == rho] and word rho's word potentials are 0, so that
// its column is a unit column.
DEV void lapl_build(float* S, LaplShared& sh, const float* __restrict__ P, int o, int n, int single_root, int rho,
                    int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const int m = n - 1, LD = LAPL_LD(m);
  // ---- normalise every word's row and write its column of A (a wave per word: the reads of P are coalesced,
  // the writes go down a column of S at the odd stride)
  for (int dp = wave; dp < m; dp += LAPL_WAVES) {
    const float* __restrict__ row = P + (long)(dp + 1) * o;
    float mx = 0.f;
    for (int j = lane; j < n; j += 64) {
      const float p = row[j];
      if (j != dp + 1 && marg_allowed(p)) mx = fmaxf(mx, p);
    }
    for (int w = 32; w >= 1; w >>= 1) mx = fmaxf(mx, __shfl_xor(mx, w));
    int e = 0;
    frexpf(mx, &e);
    float sw = 0.f, r = 0.f;
    for (int j = lane; j < n; j += 64) {
      const float p = row[j];
      if (j != dp + 1 && marg_allowed(p)) {
        const float q = ldexpf(p, -e);
        if (j == 0) r = q;
        else sw += q;
      }
    }
    for (int w = 32; w >= 1; w >>= 1) sw += __shfl_xor(sw, w);
    r = __shfl(r, 0);
    const float total = sw + r;
    if (lane == 0) {
      sh.csum[dp] = total;
      sh.cexp[dp] = (short)e;
      sh.sinv[dp] = -1;
    }
    for (int j = 1 + lane; j < n; j += 64) {
      const int hp = j - 1;
      const float p = row[j];
      float val;
      if (hp == dp) val = single_root ? sw / total : 1.f;
      else val = marg_allowed(p) ? -(ldexpf(p, -e) / total) : 0.f;
      if (single_root && hp == 0) val = r / total;
      if (rho) val = (dp == rho - 1) ? (hp == dp ? 1.f : 0.f) : (hp == dp ? sw / total : val);
      S[hp * LD + dp] = val;
    }
  }
  __syncthreads();
}

// lapl_invert: the Gauss-Jordan elimination, column by column; the inverse in
// permuted storage, the pivots in sh.pv.  Returns 2 at a pivot that is 0 or not
// finite, else 1.
DEV int lapl_invert(float* S, LaplShared& sh, int n, int tid) {
  const int lane = tid & 63;
  const int m = n - 1, LD = LAPL_LD(m);
  const int q = LAPL_THREADS / LD, rr = LAPL_THREADS - q * LD, cells = m * LD;
  const int i0 = tid / LD, j0 = tid - i0 * LD;
  for (int k = 0; k < m; ++k) {
    if (tid < ((m + 63) & ~63)) {  // whole waves
      unsigned long long key = 0;
      for (int i = lane; i < m; i += 64)
        if (sh.sinv[i] < 0) {
          const float x = S[i * LD + k];
          const float a = (x == x) ? fabsf(x) : INFINITY;  // a NaN is taken, and refused below
          const unsigned long long c = ((unsigned long long)__float_as_uint(a) << 32) | (0xFFFFFFFFu - (unsigned)i);
          key = c > key ? c : key;
        }
      for (int w = 32; w >= 1; w >>= 1) {
        const unsigned long long c = __shfl_xor(key, w);
        key = c > key ? c : key;
      }
      const int p = (int)min(0xFFFFFFFFu - (unsigned)key, (unsigned)(m - 1));
      const float piv = S[p * LD + k];
      if (tid < m) {
        sh.col[tid] = S[tid * LD + k];
        sh.prow[tid] = (tid == k ? 1.f : S[p * LD + tid]) / piv;
      }
      if (tid == 0) {
        sh.ctl[0] = p;
        sh.ctl[1] = !(fabsf(piv) > 0.f && fabsf(piv) <= FLT_MAX);
        sh.pv[k] = piv;
      }
    }
    __syncthreads();
    const int p = sh.ctl[0];
    if (sh.ctl[1]) return 2;  // (the same for every thread)
    if (tid == 0) {
      sh.sinv[p] = (short)k;
      sh.sig[k] = (short)p;
    }
    for (int x = tid, i = i0, j = j0; x < cells; x += LAPL_THREADS) {
      if (j < m) {
        const float pr = sh.prow[j];
        S[x] = (i == p) ? pr : fmaf(-sh.col[i], pr, j == k ? 0.f : S[x]);
      }
      i += q;
      j += rr;
      if (j >= LD) {
        j -= LD;
        ++i;
      }
    }
    __syncthreads();
  }
  return 1;
}

// lapl_logdet: ln Z into sh.lnz and the determinant's sign (wave 0, double,
// fixed order).  Returns 2 when the sign is not positive or ln Z not finite.
DEV int lapl_logdet(LaplShared& sh, int n, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const int m = n - 1;
  if (wave == 0) {
    double acc = 0.0;
    int neg = 0, leaders = 0;
    for (int i = lane; i < m; i += 64) {
      const float piv = sh.pv[i];
      acc += log((double)fabsf(piv)) + log((double)sh.csum[i]) + (double)sh.cexp[i] * 0.69314718055994530942;
      neg += piv < 0.f;
      int mn = i, y = sh.sig[i];  // sgn(sig) = (-1)^(m - cycles): a cycle is led by its smallest member
      for (int s = 0; s < m && y != i; ++s) {
        mn = min(mn, y);
        y = sh.sig[y];
      }
      leaders += mn == i;
    }
    for (int w = 32; w >= 1; w >>= 1) {
      acc += __shfl_xor(acc, w);
      neg += __shfl_xor(neg, w);
      leaders += __shfl_xor(leaders, w);
    }
    if (lane == 0) {
      sh.lnz = acc;
      sh.ctl[2] = ((neg + m - leaders) & 1) == 0;
    }
  }
  __syncthreads();
  const float lz = (float)sh.lnz;
  if (!sh.ctl[2] || !(fabsf(lz) <= FLT_MAX)) return 2;
  return 1;
}

// lapl_emit: the outputs, every element of [v][o] once (a wave per row).
DEV void lapl_emit(const float* S, const LaplShared& sh, const float* __restrict__ P, int o, int v, int n,
                   int single_root, float* __restrict__ marg, int* __restrict__ scores, float* __restrict__ logz,
                   int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const int m = n - 1, LD = LAPL_LD(m);
  if (tid == 0) *logz = (float)sh.lnz;
  for (int i = wave; i < v; i += LAPL_WAVES) {
    const bool word = i >= 1 && i < n;
    const int dp = i - 1;
    int srow = 0, e = 0;
    float bdd = 0.f, cs = 1.f, bd0 = 0.f;
    if (word) {
      srow = sh.sig[dp] * LD;
      bdd = S[srow + sh.sinv[dp]];
      bd0 = S[srow + sh.sinv[0]];
      cs = sh.csum[dp];
      e = sh.cexp[dp];
    }
    for (int j = lane; j < o; j += 64) {
      const long at = (long)i * o + j;
      float val = 0.f;
      bool ok = false;
      if (word && j < n && j != i) {
        const float p = P[at];
        if (marg_allowed(p)) {
          ok = true;
          const float w = ldexpf(p, -e) / cs;
          if (j == 0) {
            val = w * (single_root ? bd0 : bdd);
          } else {
            const int hp = j - 1;
            const float bdh = S[srow + sh.sinv[hp]];
            val = single_root ? (dp != 0 ? w * bdd : 0.f) - (hp != 0 ? w * bdh : 0.f) : w * (bdd - bdh);
          }
          val = fminf(1.f, fmaxf(0.f, val));
        }
      }
      marg[at] = val;
      if (scores) scores[at] = ok ? (int)rintf(val * MARG_SCALE) : TREE_FORBIDDEN;
    }
  }
}

// The matrix, its inverse and the outputs of one graph that has a tree (marg /
// scores / logz point at the graph's own outputs).  Returns 1 with the outputs
// written, 2 (nothing written) as said above.  Called by the whole workgroup.
DEV int lapl_solve(float* S, LaplShared& sh, const float* __restrict__ P, int o, int v, int n, int single_root,
                   float* __restrict__ marg, int* __restrict__ scores, float* __restrict__ logz, int tid) {
  lapl_build(S, sh, P, o, n, single_root, 0, tid);
  if (lapl_invert(S, sh, n, tid) != 1) return 2;
  if (lapl_logdet(sh, n, tid) != 1) return 2;
  lapl_emit(S, sh, P, o, v, n, single_root, marg, scores, logz, tid);
  return 1;
}

// probs [b][v][o], n_nodes [b], marg [b][v][o], logz [b], scores [b][v][o] or
// NULL, status [b]; ws: ws_stride floats per graph for the graphs with n >
// LAPL_LDS_MAXN.  grid = b, block = LAPL_THREADS.  LDS: the matrix (157,608
// B; the reachability bits, 16 KiB, lie in it before it is built) and
// LaplShared (5,656 B): 163,264 B, 163,536 as laid out, of 163,840.
__global__ void __launch_bounds__(LAPL_THREADS) k_tree_marginals(const float* __restrict__ probs, int o,
                                                                 const int* __restrict__ n_nodes, int v,
                                                                 int single_root, float* __restrict__ marg,
                                                                 float* __restrict__ logz, int* __restrict__ scores,
                                                                 int* __restrict__ status, float* ws, long ws_stride) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n = tree_node_count(n_nodes[g], v, o);
  const long base = (long)g * v * o;
  const float* __restrict__ P = probs + base;
  __shared__ float mat[LAPL_MAT_FLOATS];
  __shared__ LaplShared sh;
  static_assert(LAPL_MAT_FLOATS >= 2 * LAPL_BIT_WORDS * TREE_MAXV, "the reachability bits lie in the matrix");

  int st = 0;
  if (n >= 2) {
    int* const S = scores ? scores + base : nullptr;
    if (!lapl_has_tree((unsigned*)mat, P, o, n, single_root, tid)) st = 2;
    else if (n <= LAPL_LDS_MAXN)  // matrix in LDS or in the workspace by the graph's own n
      st = lapl_solve(mat, sh, P, o, v, n, single_root, marg + base, S, logz + g, tid);
    else
      st = lapl_solve(ws + (long)g * ws_stride, sh, P, o, v, n, single_root, marg + base, S, logz + g, tid);
  }
  if (st != 1) {  // the graph passes through: the plain arg-max downstream
    for (long x = tid; x < (long)v * o; x += LAPL_THREADS) {
      marg[base + x] = P[x];
      if (scores) scores[base + x] = TREE_FORBIDDEN;
    }
    if (tid == 0) logz[g] = st == 2 ? MARG_NEG : 0.f;
  }
  if (tid == 0) status[g] = st;
}
