// k_prop.h -- message transform + adjacency aggregation, forward and backward.
//
// Reference: compute_timestep_fast, chem_tensorflow_dense.py:391-437
//   X[g,i,:] = sum_c sum_j A[g,c,i,j] * (h[g,j,:] @ W[c] + beta[c])
// One workgroup owns one graph (the only coupling between graphs is through
// the shared weights), wave w owns the 32 hidden columns [32w, 32w+32).
#pragma once
#include "ggnn_common.h"

// cache policies: the adjacency LDS-DMA is nontemporal (each tile is read
// once per launch; measured -1.5 % on k_prop_bwd), and so are k_prop_bwd's
// dh_in loads (read once; -0.9 %).  (Nontemporal dX^T loads measured no gain.)
constexpr int kPropAAux = kNT, kPbAux = kNT;

// ===========================================================================
// k_prop_fwd: per channel c
//   MT : M_c = h W_c + beta_c                 (K = H; h from LDS, W_c from the
//                                              packed fragments in L2)
//   AGG: X  += A_c M_c                        (K = V; M_c stays in registers
//                                              as the B operand, A_c from LDS)
// LDS: h image(s) [V][H] + one A_c tile [V][V] (A_{c+1} staged by LDS-DMA
// during MT(c+1), after AGG(c) is done with the buffer).
// Outputs: X [N][H] row-major (GRU operand) and X^T [H][N] (weight-gradient
// operand, training only).
// ===========================================================================
template <int V, int H, int PREC>
__global__ void __launch_bounds__(2 * H)
k_prop_fwd(const ActT<PREC>* __restrict__ hs_in, const u16* __restrict__ Ab, const int* __restrict__ chl, int chs,
           const u16* __restrict__ Wp, long wlo,
           const float* __restrict__ beta, ActT<PREC>* __restrict__ Xo, u16* __restrict__ XT, int C, long N) {
  constexpr bool SPLIT = Prec<PREC>::split, F16 = Prec<PREC>::f16;
  using Act = ActT<PREC>;
  constexpr int NS = H / 32, NT = 64 * NS, VT = V / 32, KS = H / 16;
  constexpr int HCH = H / 8, ACH = V / 8;
  typedef Swz<ACH> SA;
  constexpr int NIMG = SPLIT ? 2 : 1;
  constexpr int IMG = V * H * 2;
  constexpr int A_BYTES = V * V * 2;
  // two adjacency tiles where the LDS has room (16-bit modes): A_{c+1} is
  // DMA'd right after channel c's only barrier, into the tile AGG(c-1) read
  constexpr int NAB = (!SPLIT && NIMG * IMG + 2 * A_BYTES <= 163840) ? 2 : 1;
  __shared__ __attribute__((aligned(16))) char smem[NIMG * IMG + NAB * A_BYTES];
  char* h_hi = smem;
  char* h_lo = smem + (SPLIT ? IMG : 0);
  auto abuf_of = [&](int i) { return smem + NIMG * IMG + (NAB == 2 ? (i & 1) * A_BYTES : 0); };

  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, ns = tid >> 6;
  const int l32 = lane & 31, hh = lane >> 5;
  const int n = ns * 32 + l32;
  const long rowg = (long)g * V;

  // channels of this graph with an edge (k_chan_list; the identity list with
  // chs = 0 for the dense loop): an empty A_c adds exactly zero, so skipping
  // it is bit-identical
  const int* cl = chl + (long)g * chs;
  const int nc = cl[0];
  auto chan = [&](int i) { return cl[1 + i]; };

  stage_rows_k<PREC, V, H, NT>(h_hi, h_lo, hs_in + rowg * H, H, tid);
  const u16* ag = Ab + (long)g * C * V * V;
  if (nc > 0) glds_tile<ACH, V, NT, kPropAAux>(abuf_of(0), ag + (long)chan(0) * V * V, tid);
  __syncthreads();
  if (NAB == 2 && nc > 1) glds_tile<ACH, V, NT, kPropAAux>(abuf_of(1), ag + (long)chan(1) * V * V, tid);

  f32x16 accx[VT];
#pragma unroll
  for (int it = 0; it < VT; ++it) accx[it] = splat(0.f);

  for (int ci = 0; ci < nc; ++ci) {
    const int c = chan(ci);
    // ---- MT: M_c[j][n] = sum_k h[j][k] W_c[k][n] + beta_c[n]
    const float bb = beta[c * H + n];
    f32x16 accm[VT];
#pragma unroll
    for (int rt = 0; rt < VT; ++rt) accm[rt] = splat(bb);
    const u16* wp = Wp + (size_t)c * H * H;
    auto ldw = [&](int ks) {
      return F2{frag_ld(wp, ns, ks, KS, lane), SPLIT ? frag_ld(wp + wlo, ns, ks, KS, lane) : frag{}};
    };
    auto mt = [&](int ks, const F2& w) {
#pragma unroll
      for (int rt = 0; rt < VT; ++rt) {
        const int off = kimg<V>(rt * 32 + l32, 2 * ks + hh);
        const frag ah = lds_frag(h_hi, off);
        const frag al = SPLIT ? lds_frag(h_lo, off) : ah;
        mma<PREC>(accm[rt], ah, al, w.a, w.b);
      }
    };
    // measured (config 3): the ring pays in the 3-product split mode, the
    // fully unrolled direct loop in the single-product modes
    if constexpr (SPLIT) b_pipeline<KS, 2>(ldw, mt);
    else b_direct<KS, KS>(ldw, mt);
    __syncthreads();  // S1: A_c visible (two tiles: and every wave is past AGG(c-1))
    if (NAB == 2 && ci >= 1 && ci + 1 < nc) glds_tile<ACH, V, NT, kPropAAux>(abuf_of(ci + 1), ag + (long)chan(ci + 1) * V * V, tid);
    const char* abuf = abuf_of(ci);
    // ---- AGG: X[i][n] += sum_j A_c[i][j] M_c[j][n]
#pragma unroll
    for (int rt = 0; rt < VT; ++rt) {
      const frag mh0 = acc_hi<F16>(accm[rt], 0), mh1 = acc_hi<F16>(accm[rt], 1);
      const frag ml0 = SPLIT ? acc_lo<F16>(accm[rt], 0) : mh0, ml1 = SPLIT ? acc_lo<F16>(accm[rt], 1) : mh1;
#pragma unroll
      for (int it = 0; it < VT; ++it) {
        const frag a0 = lds_frag(abuf, SA::off(it * 32 + l32, 4 * rt + hh));
        const frag a1 = lds_frag(abuf, SA::off(it * 32 + l32, 4 * rt + 2 + hh));
        mma_xa<PREC>(accx[it], a0, mh0, ml0);
        mma_xa<PREC>(accx[it], a1, mh1, ml1);
      }
    }
    if constexpr (NAB == 1) {
      __syncthreads();  // S2: A_c reads done
      // A_{c+1} lands in LDS by DMA while MT(c+1) runs (drained by its S1)
      if (ci + 1 < nc) glds_tile<ACH, V, NT, kPropAAux>(abuf_of(0), ag + (long)chan(ci + 1) * V * V, tid);
    }
  }

  // ---- X^T (transposed, weight-gradient operand)
  if (XT) {
#pragma unroll
    for (int it = 0; it < VT; ++it)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        st_col4w<PREC>(XT + wg_off(n, rowg + it * 32 + 4 * hh, H) + 8 * q, accx[it][4 * q], accx[it][4 * q + 1],
                       accx[it][4 * q + 2], accx[it][4 * q + 3]);
  }
  // ---- X row-major through LDS (the h images are free once every wave is past the last MT)
  if constexpr (SPLIT) {
    float* xs = (float*)smem;  // [V][H] fp32 = NIMG*IMG bytes
#pragma unroll
    for (int it = 0; it < VT; ++it)
#pragma unroll
      for (int r = 0; r < 16; ++r) xs[(it * 32 + acc_row(r, hh)) * H + n] = accx[it][r];
    __syncthreads();
    for (int q = tid; q < V * H / 4; q += NT) *(float4*)(Xo + rowg * H + q * 4) = ((const float4*)xs)[q];
  } else {
#pragma unroll
    for (int it = 0; it < VT; ++it)
#pragma unroll
      for (int r = 0; r < 16; ++r) *(u16*)(h_hi + kimg<V>(it * 32 + acc_row(r, hh), n >> 3) + (n & 7) * 2) = to_limb<F16>(accx[it][r]);
    __syncthreads();
    for (int q = tid; q < V * HCH; q += NT) {
      const int row = q / HCH, ch = q % HCH;
      st16(Xo + (rowg + row) * H + ch * 8, ld16(h_hi + kimg<V>(row, ch)));
    }
  }
}

// ===========================================================================
// k_prop_bwd: backward of message + aggregation, per channel c
//   dM_c^T[n][j] = sum_i dX^T[n][i] A_c[i][j]    (K = V; dX^T fragments stay in
//                                                registers for all channels)
//   dM_c -> LDS [j][n] image(s); dM_c^T -> HBM (weight-gradient operand)
//   dh[j][k]   += sum_n dM_c[j][n] W_c[k][n]     (K = H)
//   dbeta_c[n] += sum_i deg_c[i] dX[i][n]        (= sum_j dM_c[j][n]; per-graph
//                                                partials dbp [b][C][H])
// ===========================================================================
template <int V, int H, int PREC>
__global__ void __launch_bounds__(2 * H)
k_prop_bwd(const ActT<PREC>* __restrict__ dXT, const u16* __restrict__ AbT, const u16* __restrict__ deg,
           const int* __restrict__ chl, int chs, const u16* __restrict__ WTp, long wlo, const float* __restrict__ dh_in, float* __restrict__ dh_out,
           u16* __restrict__ dMT, float* __restrict__ dbp, int C, long N, Drop dr, int tm,
           const uint32_t* __restrict__ gmax, int zdm, const uint2* __restrict__ sbits) {
  // sbits: the forward's state keep bits of timestep tm (k_fwd_fused,
  // FusedFwdArgs::sbits; this kernel's lane / tile mapping is the same), or
  // null: the mask's Philox blocks are drawn here
  dr = drop_resolve(dr);  // (a device-resident key: loaded once)
  TSCLK(3, 0);
  // phase stamps (GGNN_TS build, tools/ts_probe.py), in the order they are taken:
  // 0 start, 4 dX^T fragments built and the dbeta product done, 1 prologue barrier
  // passed (first A tile, keep bits), then of the LAST non-empty channel 2 its
  // start, 3 phase a, 5 S1 + phase b, 6 dM^T stores issued; 7 epilogue done
  TSMARK(3, 0);
  constexpr bool SPLIT = Prec<PREC>::split, F16 = Prec<PREC>::f16;
  using Act = ActT<PREC>;
  constexpr int NS = H / 32, NT = 64 * NS, VT = V / 32, KV = V / 16, KS = H / 16;
  constexpr int HCH = H / 8, ACH = V / 8;
  typedef Swz<HCH> SH;
  typedef Swz<ACH> SA;
  constexpr int NIMG = SPLIT ? 2 : 1;
  constexpr int IMG = V * H * 2, A_BYTES = V * V * 2;
  __shared__ __attribute__((aligned(16))) char smem[A_BYTES + NIMG * IMG];
  char* abuf = smem;
  char* m_hi = smem + A_BYTES;
  char* m_lo = m_hi + (SPLIT ? IMG : 0);

  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, ns = tid >> 6, l32 = lane & 31, hh = lane >> 5;
  const int n = ns * 32 + l32;
  const long rowg = (long)g * V;

  // dX^T fragments of this wave's 32 columns (A operand of the dM^T product)
  frag dxh[KV], dxl[KV];
#pragma unroll
  for (int s = 0; s < KV; ++s) {
    const Act* p = dXT + wg_off(n, rowg + 16 * s + 8 * hh, H);  // K-blocked (ggnn_common.h)
    if constexpr (SPLIT) {
      typedef float f4v __attribute__((ext_vector_type(4)));
      const f4v a = *(const f4v*)p, b = *(const f4v*)(p + 4);
      const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      dxh[s] = pk8<true>(x);
      dxl[s] = pk8_lo<true>(x);
    } else {
      dxh[s] = ld16(p);
      dxl[s] = dxh[s];
    }
  }

  // non-empty channels only (k_chan_list); the others get dM = 0 (end of kernel)
  const int* cl = chl + (long)g * chs;
  const int nc = cl[0];
  auto chan = [&](int i) { return cl[1 + i]; };
  const u16* ag = AbT + (long)g * C * V * V;
  if (nc > 0) glds_tile<ACH, V, NT, kPropAAux>(abuf, ag + (long)chan(0) * V * V, tid);
  const rsrc_t rdh = mkrsrc(dh_in + rowg * H, V * H * 4);
  const int vo = (4 * hh * H + n) * 4;
  // the forward's state keep bits of timestep tm, loaded here so the
  // epilogue's stores do not wait for them
  const bool drop = dr.thr != 0 && tm >= 0;
  uint2 kb = make_uint2(0u, 0u);
  if (drop && sbits) kb = sbits[((long)tm * gridDim.x + g) * NT + tid];
  if (dbp) {
    // dbeta_c[n] = sum_i dX[i][n] deg_c[i] as one more MFMA product, once per launch:
    // output column l32 of group grp belongs to the graph's non-empty channel
    // chan(32 grp + l32), B[i][l32] = deg_c[i] (exact integers; zeros past nc).  MFMA
    // columns are independent, so each partial has the bits of a product whose 32
    // columns all carried one channel's deg (what ran once per channel, between phase
    // a and S1, until this was moved: 1.4-1.7 us of every channel's chain,
    // profiles/prop_bwd_launch_before.log).  Here it runs while the first A tile is
    // in flight.  Per-graph partials [b][C][H] (no atomics); reduced over graphs
    // after the last step.
    // (Round 6 tried the column sums of the dM^T accumulators instead -- a lane
    // butterfly, 16 fewer MFMAs per channel and wave -- and the extra live
    // registers spilled 29-69 VGPRs at 256: not kept.)
#pragma unroll 1
    for (int grp = 0; 32 * grp < nc; ++grp) {
      const int li = 32 * grp + l32;
      const bool live = li < nc;
      // (a column past the list's end loads the degrees of the list's first channel and
      // drops them: in bounds, and no branch around the loads)
      const int c = chan(live ? li : 0);
      const u16* dg = deg + ((long)g * C + c) * V + 8 * hh;
      frag dq[KV];
#pragma unroll
      for (int ss = 0; ss < KV; ++ss) {
        const frag d = ld16(dg + 16 * ss);
        dq[ss] = live ? d : make_uint4(0, 0, 0, 0);
      }
      f32x16 db = splat(0.f);
#pragma unroll
      for (int ss = 0; ss < KV; ++ss) mma_xb<PREC>(db, dxh[ss], dxl[ss], dq[ss]);
      // lane (l32, hh) holds rows 8 q + 4 hh .. + 3 of its channel in registers 4 q .. 4 q + 3
      if (live) {
        float* o = dbp + ((long)g * C + c) * H + ns * 32 + 4 * hh;
#pragma unroll
        for (int q = 0; q < 4; ++q) *(float4*)(o + 8 * q) = make_float4(db[4 * q], db[4 * q + 1], db[4 * q + 2], db[4 * q + 3]);
      }
    }
  }
  TSMARK(3, 4);
  __syncthreads();  // dX^T fragments built, first A tile and keep bits landed
  TSMARK(3, 1);
  // dL/dh_t, the C operand of phase b: loaded behind the barrier, so that the barrier's
  // vmcnt(0) does not wait for it; it lands under channel 0's phase a and is first
  // waited for in phase b (nothing in phase a waits on vmcnt).  With nc == 0 it passes
  // straight to the epilogue.
  f32x16 adh[VT];
#pragma unroll
  for (int jt = 0; jt < VT; ++jt)
#pragma unroll
    for (int r = 0; r < 16; ++r) adh[jt][r] = bld_p<kPbAux>(rdh, vo, (jt * 32 + acc_row0(r)) * H * 4);

  for (int ci = 0; ci < nc; ++ci) {
    const int c = chan(ci);
    TSMARK(3, 2);
    // Split mode: A_{c+1} is loaded into registers here (NAP x 16 bytes per lane, the
    // source addresses of the tile's DMA) and flies under phase a; LDS is full, so it is
    // written to abuf only after S1, when every wave is done with A_c.  Phase b then has
    // nothing but its weight fragments on vmcnt.  (Until this, the tile went out as an
    // LDS-DMA after S1, its lines touched into L2 from here, and phase b's first fragment
    // wait covered it: profiles/prop_bwd_phase_b_ab.log, prop_bwd_launch_ab.log.)
    constexpr int NAP = (V * ACH + NT - 1) / NT;
    uint4 an[NAP] = {};
    if constexpr (SPLIT) {
      if (ci + 1 < nc) tile_ld<ACH, V, NT, kPropAAux>(an, ag + (long)chan(ci + 1) * V * V, tid);
    }
    // ---- phase a: dM_c^T tile (rows n of this wave), one 32-column j tile at a time.
    // Two tiles in flight: tile jt's accumulator is converted and written to the LDS
    // images in NP pieces, one behind each MFMA of tile jt+1's chain (the wave
    // issues in order: conversions placed after a whole chain wait for it, and the
    // next chain waits for them).  The sched_barriers pin that interleaving; left
    // alone the scheduler hoists all VT chains ahead of the conversions (64
    // accumulator VGPRs live, spills at 128 x 256).  A_c's fragments run two MFMA
    // steps ahead of their use.
    {
      constexpr int NST = VT * KV;               // MFMA steps (one A_c fragment each)
      constexpr int NM = SPLIT ? 2 : 1;          // MFMAs per step
      constexpr int NP = 16 / (KV * NM);         // conversion pieces behind each MFMA (16 per tile)
      auto lda = [&](int i) { return lds_frag(abuf, SA::off((i / KV) * 32 + l32, 2 * (i % KV) + hh)); };
      frag bq[2] = {lda(0), lda(NST > 1 ? 1 : 0)};
      f32x16 am[2];
      uint32_t pq[2] = {0u, 0u};
      float lq[2] = {0.f, 0.f};
      // piece t of a tile: quad q = t >> 2 (registers 4q .. 4q+3: rows n0 .. n0+3 of column j)
      //   0: the 16-bit limbs -> m_hi    1: e5m2(dM) -> m_lo
      //   2, 3: the limbs' residuals (one rounding: against the pairs packed in piece 0) 2^F8_M -> m_lo
      auto piece = [&](int jt, int t, const f32x16& x) {
        const int q = t >> 2, k = t & 3, j = jt * 32 + l32;
        const int o = 8 * q + 4 * hh;  // this quad's offset inside the wave's 32 columns
        const int m8 = kimg<V>(j, 4 * ns + (o >> 4)) + (o & 15);
        if (k == 0) {
          const int n0 = ns * 32 + o;
          pq[0] = pk<F16>(x[4 * q], x[4 * q + 1]);
          pq[1] = pk<F16>(x[4 * q + 2], x[4 * q + 3]);
          *(uint2*)(m_hi + kimg<V>(j, n0 >> 3) + (n0 & 7) * 2) = make_uint2(pq[0], pq[1]);  // chunk-major dM image
        }
        if constexpr (SPLIT) {
          // fp8 correction image (mfma_f8corr's A operand): per row j and 32-column
          // block ns, 4 chunks [e5m2(dM) n 0-15 | n 16-31 | e5m2(dM_lo 2^F8_M) n 0-15 | n 16-31]
          const float sc = (float)(1 << F8_M);
          if (k == 1) *(uint32_t*)(m_lo + m8) = pk4_bf8(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
          if (k == 2) {
            lq[0] = resid16<0>(x[4 * q], pq[0]) * sc;
            lq[1] = resid16<1>(x[4 * q + 1], pq[0]) * sc;
          }
          if (k == 3)
            *(uint32_t*)(m_lo + m8 + 2 * V * 16) =
                pk4_bf8(lq[0], lq[1], resid16<0>(x[4 * q + 2], pq[1]) * sc, resid16<1>(x[4 * q + 3], pq[1]) * sc);
        }
      };
#pragma unroll
      for (int i = 0; i < NST; ++i) {
        const int jt = i / KV, s = i % KV;
        f32x16& acc = am[jt & 1];
        if (s == 0) acc = splat(0.f);
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          // (mma_xb's order: the lo limb's product first)
          if (SPLIT && m == 0) acc = mfma<true>(dxl[s], bq[i & 1], acc);
          else acc = mfma<F16>(dxh[s], bq[i & 1], acc);
          if (m == NM - 1 && i + 2 < NST) bq[i & 1] = lda(i + 2);
          if (jt > 0) {
#pragma unroll
            for (int t = (s * NM + m) * NP; t < (s * NM + m + 1) * NP; ++t) piece(jt - 1, t, am[(jt - 1) & 1]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int t = 0; t < 16; ++t) piece(VT - 1, t, am[(VT - 1) & 1]);
    }
    TSMARK(3, 3);
    __syncthreads();  // S1: dM images complete, A_c reads done
    // A_{c+1} into abuf, published by S2.  Split mode: from the registers loaded at the top
    // of the channel (ds_write_b128, the slots the DMA would fill; the compiler's vmcnt(0)
    // in front of it also covers the previous channel's dM^T stores, a phase a old by
    // now).  16-bit modes: by DMA while phase b runs, as before
    if (ci + 1 < nc) {
      if constexpr (SPLIT) tile_st<ACH, V, NT>(abuf, an, tid);
      else glds_tile<ACH, V, NT, kPropAAux>(abuf, ag + (long)chan(ci + 1) * V * V, tid);
    }
    // ---- phase b: dh[j][k] += sum_n dM_c[j][n] W_c^T[n][k]
    const u16* wt = WTp + (size_t)c * H * H;
    // Split mode: dM and W_c^T both as hi + lo (round 5's hi-only W_c^T reached
    // 1.07e-3 of the 1e-3 bar, tests/test_precision_policies.py); since round 6
    // the two correction terms run on the fp8 MFMA (4 instead of 6 cycle units
    // per 32 k; their error is 2^-15 of the product against 2^-12 for a dropped
    // limb: the gradients' error does not move, tools/precision_policies.py --hybrid)
    if constexpr (SPLIT) {
      // per 32-column block kb of dM: the hi product on two 32x32x16 f16 MFMAs,
      // both limb corrections on one fp8 32x32x64 (mfma_f8corr; W_c^T's
      // correction fragments sit where its f16 lo limbs would, k_pack_multi f8)
      // The fragment ring alternates the block's two halves (the f16 hi fragments
      // of k-steps 2kb, 2kb+1; the 32-byte fp8 fragment), 8 cycle units each: the
      // same 2 x 8 VGPRs in flight as the 3-product ring (b_pipeline<KS, 2>)
      const char* w8 = (const char*)(wt + wlo);
      auto ld_h = [&](int kb) { return F2{frag_ld(wt, ns, 2 * kb, KS, lane), frag_ld(wt, ns, 2 * kb + 1, KS, lane)}; };
      auto ld_f = [&](int kb) {
        const uint4* f = (const uint4*)(w8 + ((size_t)(ns * (KS / 2) + kb) * 64 + lane) * 32);
        return F2{f[0], f[1]};
      };
      constexpr int NKB = KS / 2;
      typedef std::integral_constant<bool, false> NotLast;
      typedef std::integral_constant<bool, true> Last;
      // each half waits only for its own fragment (vmcnt(2): the other half's two loads
      // stay in flight); the last k-block is peeled and loads nothing
      F2 rh = ld_h(0), rf = ld_f(0);
      auto blk = [&](int kb, auto last) {
        constexpr bool LAST = decltype(last)::value;
#pragma unroll
        for (int jt = 0; jt < VT; ++jt) {
          const int row = jt * 32 + l32;
          adh[jt] = mfma<true>(lds_frag(m_hi, kimg<V>(row, 4 * kb + hh)), rh.a, adh[jt]);
          adh[jt] = mfma<true>(lds_frag(m_hi, kimg<V>(row, 4 * kb + 2 + hh)), rh.b, adh[jt]);
        }
        if (!LAST) rh = ld_h(kb + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int jt = 0; jt < VT; ++jt) {
          const int row = jt * 32 + l32;
          const uint4 p0 = ld16(m_lo + kimg<V>(row, 4 * kb + 2 * hh)), p1 = ld16(m_lo + kimg<V>(row, 4 * kb + 2 * hh + 1));
          adh[jt] = mfma_f8corr(p0, p1, rf.a, rf.b, adh[jt]);
        }
        if (!LAST) rf = ld_f(kb + 1);
        __builtin_amdgcn_sched_barrier(0);
      };
#pragma unroll 1
      for (int kb = 0; kb < NKB - 1; ++kb) blk(kb, NotLast());
      blk(NKB - 1, Last());
      // (register-only MFMAs may be sunk past the stores and S2 into the next channel,
      // and the last fp8 fragment's wait with them: it would then cover the stores)
#pragma unroll
      for (int jt = 0; jt < VT; ++jt) asm volatile("" : "+v"(adh[jt])::"memory");
    } else {
      auto ldb = [&](int ks) { return F2{frag_ld(wt, ns, ks, KS, lane), frag{}}; };
      auto pb = [&](int ks, const F2& w) {
#pragma unroll
        for (int jt = 0; jt < VT; ++jt) {
          const frag ah = lds_frag(m_hi, kimg<V>(jt * 32 + l32, 2 * ks + hh));
          mma<PREC>(adh[jt], ah, ah, w.a, w.b);
        }
      };
      b_pipeline<KS, 2, 1>(ldb, pb);  // rolled ring: measured 3.5 % over b_direct / full unroll (spills)
    }
    TSMARK(3, 5);
    // dM_c^T -> HBM [c][n][N] (weight-gradient operand), read back from the
    // 16-bit image m_hi (complete since S1; it holds the bits the stores carry) with
    // the transposing LDS read, so phase a keeps no copy in registers.  Issued after
    // the last weight-fragment wait of the channel: vmcnt is in order, so a store
    // ahead of a load would make that load's wait cover the store too.  The stores
    // then drain during the next channel's phase a, whose only vector-memory loads are
    // the split mode's loads of A_{c+2} (consumed after S1, not there).
    // 16 contiguous bytes (8 j of one n) per lane, (8-byte stores are issue-bound:
    // ~7 B/cycle/CU, 16-byte ones about twice that); a 32-lane half writes whole
    // 64-byte lines of 8 n.  Per store s, half hh takes chunk 4 ns + 2 s + hh; its
    // 16-lane group gb the tile's rows 16 gb .. 16 gb + 15: lane 4q + p of a group
    // supplies row 8 (p >> 1) + 4 r + q, bytes 8 (p & 1) .. +7 of the chunk, and
    // lane i receives n = 8 chunk + (i & 7), rows 8 (i >> 3) + 4 r .. + 3.  Group 1
    // reads its r = 1 rows first: one instruction's 32 lanes of a half then cover
    // all 64 banks once (rows {0-3, 8-11} and {20-23, 28-31}: no conflict).
    // global_store, not buffer_store: the raw-buffer dwordx4 store read its data
    // VGPRs late (DESIGN.md §4 lessons).
    if (dMT) {
      // lane addresses of the two reads inside a (32 j x 16 n) piece of m_hi and of
      // the store, recomputed per channel from an opaque copy of the lane id: kept
      // live across phases a and b they cost five VGPRs there
      int ln = lane;
      asm volatile("" : "+v"(ln));
      const int gb = (ln >> 4) & 1, i16 = ln & 15, h2 = ln >> 5;
      const int trx = kimg<V>(16 * gb + 8 * ((i16 >> 1) & 1) + 4 * gb + (i16 >> 2), h2) + 8 * (i16 & 1);
      const int try_ = trx ^ 64;  // the other 4-row block
      u16* dmt = dMT + (long)c * H * N + wg_off(ns * 32 + 8 * h2 + (i16 & 7), rowg + 16 * gb + 8 * (i16 >> 3), H);
#pragma unroll
      for (int jt = 0; jt < VT; ++jt)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const char* src = m_hi + kimg<V>(jt * 32, 4 * ns + 2 * s);
          const v2u32 x = lds_tr16(src + trx), y = lds_tr16(src + try_);
          typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));
          const u32x4v out = gb ? u32x4v{y.x, y.y, x.x, x.y} : u32x4v{x.x, x.y, y.x, y.y};
          __builtin_nontemporal_store(out, (u32x4v*)(dmt + wg_off(16 * s, jt * 32, H)));
        }
    }
    TSMARK(3, 6);
    __syncthreads();  // S2: dM image reads done, A_{c+1} staged
  }
  const rsrc_t rdo = mkrsrc(dh_out + rowg * H, V * H * 4);
  // dL/dh_t -> dL/dh'_{t-1} through the state dropout of timestep tm = t-1
  const float osc = gunscale(gmax);  // last step writing dL/dh0 in place: undo the gradient scale, else 1
#pragma unroll
  for (int jt = 0; jt < VT; ++jt) {
    uint4 dw = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float x = adh[jt][r] * osc;
      if (drop) {
        if (sbits) {
          const uint32_t w = (VT == 4) ? ((jt >> 1) ? kb.y : kb.x) : kb.x;
          x = ((w >> ((jt & 1) * 16 + r)) & 1u) ? x * dr.scale : 0.0f;
        } else {
          if ((r & 3) == 0) dw = state_words(dr, g, jt * 32 + acc_row0(r) + 4 * hh, n, tm);
          x = drop_apply(dr, u4_get(dw, r & 3), x);
        }
      }
      bst(rdo, x, vo, (jt * 32 + acc_row0(r)) * H * 4);
    }
  }
  // empty channels: dM_c = A_c^T dX = 0 exactly.  Their dbeta partials are
  // written as zeros, and so are their dM^T rows (the graph's V*H contiguous
  // elements of channel c, wg_off layout) when the weight-gradient kernel
  // reads every row (zdm; with per-channel graph lists it skips them)
  if (nc < C) {
    for (int c = 0, p = 0; c < C; ++c) {
      if (p < nc && cl[1 + p] == c) {
        ++p;
        continue;
      }
      if (dMT && zdm) {
        u16* z = dMT + (long)c * H * N + rowg * H;
        for (int q = tid; q < V * H / 8; q += NT) st16(z + q * 8, make_uint4(0, 0, 0, 0));
      }
      if (dbp)
        for (int q = tid; q < H; q += NT) dbp[((long)g * C + c) * H + q] = 0.f;
    }
  }
  TSMARK(3, 7);
  TSCLK(3, 1);
}
