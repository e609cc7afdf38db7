/*
 * ggnn.h -- C ABI of the MI355X-native GGNN propagation engine (libggnn.so).
 *
 * Drop-in boundary for the reference's hot path
 *   DenseGGNNChemModel.compute_final_node_representations
 *   (crismolav/ggnn, chem_tensorflow_dense.py:312-340, called from
 *    chem_tensorflow.py:319-322)
 * together with its TF-autodiff backward (chem_tensorflow.py:496).
 *
 * The reference has no FFI: the path is a Python template method that builds
 * TensorFlow ops.  Each entry point below replaces one piece of that method:
 *
 *   ggnn_pack_weights   <- the path's variables, chem_tensorflow_dense.py:202-212
 *                          (edge_weights [C,h,h], edge_biases [C,1,h]) and the
 *                          GRUCell kernels/biases built at :237-241
 *   ggnn_set_adjacency  <- the adjacency placeholder + transpose, :192-195
 *                          (feed [b, C, v, v], row = receiving node, :65-83)
 *   ggnn_forward        <- the T-step loop, :312-340 = compute_timestep_fast
 *                          (:391-437) + GRUCell (:333), returns [b, v, h]
 *   ggnn_backward       <- TF autodiff of the same loop (chem_tensorflow.py:496):
 *                          dL/dh0 and the weight gradients (before clip/Adam)
 *   ggnn_dims.edge_keep / state_keep / seed
 *                       <- tf.nn.dropout of the edge weights (:397-403) and the
 *                          GRUCell DropoutWrapper (:239-240), fed at :860-861
 *
 * Conventions
 *  - Every tensor argument is a raw device pointer (hipMalloc'd or any HIP
 *    allocator, e.g. PyTorch-ROCm tensors used only as memory holders).
 *  - Host-visible layouts are the reference's: row-major fp32,
 *      adjacency [b][C][v][v] (0/1 values, row = receiver, col = sender),
 *      h0 / hT / dhT / dh0 [b][v][h],
 *      edge_weights [C][h][h] (in x out), edge_biases [C][h],
 *      gates_kernel [2h][2h] (rows [x ; h], cols [r | u]), gates_bias [2h],
 *      candidate_kernel [2h][h] (rows [x ; r*h]), candidate_bias [h].
 *  - The caller owns all memory.  The library never allocates: it works
 *    inside a caller-provided workspace sized by ggnn_workspace_bytes and a
 *    weight pack sized by ggnn_weight_pack_bytes.
 *  - All calls are asynchronous and stream-ordered on `stream`; they are safe
 *    to capture into a hipGraph (no sync, no malloc inside).
 *  - Return value: 0 on success, negative GGNN_E* on error; a description of
 *    the last error of the calling thread is in ggnn_last_error().
 *    No exception or abort crosses the ABI.
 */
#ifndef GGNN_H
#define GGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ggnn_stream_t; /* hipStream_t (0 = default stream) */

enum {
  GGNN_OK = 0,
  GGNN_EINVAL = -1,    /* invalid dims / null pointer */
  GGNN_EUNSUP = -2,    /* dims outside the compiled kernel set */
  GGNN_ELAUNCH = -3,   /* HIP launch / runtime error */
  GGNN_EALIGN = -4     /* pointer alignment */
};

/* flags */
#define GGNN_USE_EDGE_BIAS 1 /* params['use_edge_bias'], chem_tensorflow_dense.py:158 */
/* Precision policy (fp32 accumulation in every mode).
 *   default (0)       bf16 MFMA operands, bf16 activations between kernels
 *   GGNN_FP16         f16 MFMA operands (3 more mantissa bits, same rate)
 *   GGNN_FP32_PARITY  every non-exact operand carried as an f16 hi/lo limb
 *                     pair (3 MFMAs per product, ~22-bit operand mantissa),
 *                     fp32 activations: matches the reference's fp32
 *                     arithmetic to <= 1e-3 (tests/test_gpu_parity.py).  The
 *                     backward's dz W^T / dM W_c^T products run their limb
 *                     corrections on the block-scaled fp8 MFMA (e5m2 x e4m3;
 *                     DESIGN.md §8.5); the forward keeps three f16 MFMAs */
#define GGNN_FP32_PARITY 2
#define GGNN_FP16 4
/* Empty-channel skipping.  The staged adjacency carries a
 * per-graph list of the channels with at least one edge; the message
 * transform and aggregation (forward and backward) run only over those, since
 * an empty A[g,c] contributes exactly zero (the real btb adjacency has
 * C = 2E = 92 channels, about 60 % of them empty per graph).  Results are
 * bit-identical to the dense loop.  GGNN_DENSE_CHANNELS turns the skipping
 * off (A/B measurement and the bit-identity test). */
#define GGNN_DENSE_CHANNELS 8
/* The general path (k_gemm.h + k_generic.h): any hidden size and vertex count.
 * Taken automatically when hidden is not 128 / 256 or v > 128 (e.g. the
 * reference's default hidden_size 400, chem_tensorflow.py:95, and its
 * 198-node buckets, chem_tensorflow_dense.py:584-585); GGNN_GENERIC forces it
 * for every shape (parity tests, A/B). */
#define GGNN_GENERIC 16
/* Run the forward of hidden 256, v <= 128 batches as per-timestep k_prop_fwd +
 * k_gru_fwd launches instead of the one-launch fused forward (A/B and tests). */
#define GGNN_UNFUSED_FWD 32

/* Sparse message passing on the general path ("pair mode", k_pairs.h): the
 * message transform runs over the (node, channel) pairs with an incoming edge
 * (X = sum_c (A_c h) W_c + deg beta_c, re-associated) instead of over every
 * row of every non-empty (graph, channel) tile -- the reference's dependency
 * trees have ~4 such pairs per node against ~26 non-empty channels per graph
 * (C = 92).  Same results as the dense loop up to fp32 summation order.
 * Implies GGNN_GENERIC; needs hidden % 4 == 0 and a batch staged by
 * ggnn_set_adjacency_edges with num_edges <= b * v (every edge adds at most
 * 4 pairs, so the pair buffers hold 4 * b * v rows plus channel padding);
 * ggnn_set_adjacency rejects it. */
#define GGNN_SPARSE_PAIRS 64
/* Dropout seeds live in device memory: dims.seed (and the `seed` argument of
 * ggnn_embed_* / ggnn_heads_*) holds the ADDRESS of a device uint64 that the
 * kernels read when they run, instead of the seed itself.  A step captured in
 * a hipGraph then replays with whatever seed the caller wrote there (by a
 * captured copy) -- no re-capture per training step.  Same masks as passing
 * that value directly. */
#define GGNN_SEED_DEVICE 128

typedef struct ggnn_dims {
  int32_t b;     /* graphs in the batch      (placeholders['num_graphs'])   */
  int32_t v;     /* vertices per graph       (placeholders['num_vertices']) */
  int32_t h;     /* hidden size              (params['hidden_size'])        */
  int32_t C;     /* adjacency channels = 2 * num_edge_types                 */
  int32_t T;     /* timesteps (params['num_timesteps'] or fixed_ts)         */
  int32_t flags; /* GGNN_USE_EDGE_BIAS | GGNN_FP32_PARITY or GGNN_FP16      */
  /* Dropout (applied whenever keep < 1, as the reference applies it whenever
   * a keep probability < 1 is fed; it feeds 1.0 at evaluation, :938-940):
   *   edge_keep  = placeholders['edge_weight_dropout_keep_prob']: every
   *                timestep multiplies W by a fresh mask / keep (:397-403);
   *   state_keep = placeholders['graph_state_keep_prob']: DropoutWrapper
   *                state dropout of every new GRU state (:239-240).
   * Both must lie in (0, 1].  Masks are Philox4x32-10 keyed by `seed`
   * (DESIGN.md "Dropout"), so pack, forward and backward of one step must
   * see the same seed; draw a new seed per training step. */
  float edge_keep;
  float state_keep;
  uint64_t seed;
} ggnn_dims;

int ggnn_version(void);
const char* ggnn_last_error(void);

/* Validate dims: b, v, C, T >= 1, 1 <= h <= 4096, C <= 4096.  hidden 128 / 256
 * with v <= 128 run the specialised kernels, every other shape the general
 * path.  Returns 0 or GGNN_EUNSUP / GGNN_EINVAL. */
int ggnn_check_dims(const ggnn_dims* d);

/* Bytes of the per-batch workspace (activations saved for backward when
 * training != 0), of one staged adjacency batch and of one weight pack.
 * The workspace size depends on b, v, h, C, T, flags, training and on whether
 * edge dropout is on (edge_keep < 1), not on state_keep or the seed: one
 * workspace serves every state-dropout setting of its shape. */
int ggnn_workspace_bytes(const ggnn_dims* d, int training, size_t* bytes);
int ggnn_adjacency_bytes(const ggnn_dims* d, size_t* bytes);
int ggnn_weight_pack_bytes(const ggnn_dims* d, size_t* bytes);

/* Convert fp32 master weights into the engine's MFMA fragment layouts, in the
 * precision policy of d->flags: bf16 (flag 0), f16 (GGNN_FP16) or an f16
 * hi/lo limb pair per element (GGNN_FP32_PARITY; the backward's transposed
 * packs carry e4m3 correction fragments in place of the lo limbs, clamped to
 * +-448 after their power-of-two scaling); plus the fp32 bias copies
 * and the general path's fp32 weight copies (one per timestep under edge
 * dropout, masked).  edge_biases may be NULL when !(flags & GGNN_USE_EDGE_BIAS). */
int ggnn_pack_weights(const ggnn_dims* d, void* pack,
                      const float* edge_weights, const float* edge_biases,
                      const float* gates_kernel, const float* gates_bias,
                      const float* candidate_kernel, const float* candidate_bias,
                      ggnn_stream_t stream);

/* The same pack for the batch staged in `adj` (d: that batch's dims).  On the
 * general path under edge dropout it writes the per-timestep masked copies of
 * W_c only for the channels with an edge somewhere in the batch (the others
 * are never read by that batch's forward / backward: tf.nn.dropout of
 * edge_weights, chem_tensorflow_dense.py:397-403, touches only weights the
 * batch uses).  Everything else, and other paths, as ggnn_pack_weights.  The
 * pack then serves THAT staged batch only. */
int ggnn_pack_weights_batch(const ggnn_dims* d, void* pack, const void* adj,
                            const float* edge_weights, const float* edge_biases,
                            const float* gates_kernel, const float* gates_bias,
                            const float* candidate_kernel, const float* candidate_bias,
                            ggnn_stream_t stream);

/* Test / tuning hook: D[M][N] = A[M][K] B[K][N], row-major fp32 device
 * buffers, through the general path's MFMA product kernel (k_gemm) in the
 * precision policy of d->flags (other fields of d: any valid dims). */
int ggnn_dbg_gemm(const ggnn_dims* d, int M, int N, int K, const float* A, const float* B, float* D,
                  ggnn_stream_t stream);

/* The same with every operand layout the general path uses:
 *   a_layout 0: A fp32 [M][K]; 1: A fp32 [K][M]; 2: A 16-bit limbs [M][K]
 *               (exact values: 0/1 adjacency; f16 in the fp16 / fp32 modes)
 *   b_layout 0: B fp32 [K][N]; 1: B fp32 [N][K]
 *   kernel   0: automatic; 1: k_gemm; 2: k_gemm_ring without the K split
 *               over waves; 3 / 4 / 5: k_gemm_ks (the K split) with 1 / 2 / 4
 *               column blocks of 32 (fp32 k-contiguous A).  2-5 return
 *               GGNN_EINVAL if the operands do not meet the ring's alignment
 *               rules */
int ggnn_dbg_gemm_ex(const ggnn_dims* d, int M, int N, int K, const void* A, int a_layout, const float* B,
                     int b_layout, float* D, int kernel, ggnn_stream_t stream);

/* Stage one batch's adjacency [b][C][v][v] fp32 (0/1) into `adj` (sized by
 * ggnn_adjacency_bytes): 16-bit (exact for 0/1; bf16, or f16 under GGNN_FP16 /
 * GGNN_FP32_PARITY), its transpose, per-node in-degrees and the per-graph list
 * of non-empty channels.  T of d is ignored. */
int ggnn_set_adjacency(const ggnn_dims* d, void* adj, const float* adjacency,
                       ggnn_stream_t stream);

/* Stage one batch's adjacency from edge lists instead of the dense feed (the
 * compact producer of SURVEY §8f): the same staged bytes as
 * ggnn_set_adjacency(graph_to_adj_mat_bd(...)) (chem_tensorflow_dense.py:65-83,
 * built per graph at :539) without the [b][2E][v][v] host array or its copy.
 *   edges         device int32 [num_edges][3] = (src, label, dest) rows of the
 *                 reference's 'graph' lists, graphs concatenated;
 *   graph_offsets device int32 [b + 1]: graph g owns rows [off[g], off[g+1]);
 *   num_edge_types E with d->C == 2E.
 * Labels outside 1..E or nodes outside 0..v-1 are skipped (validate on the
 * host: the reference raises IndexError for them). */
int ggnn_set_adjacency_edges(const ggnn_dims* d, void* adj, const int32_t* edges,
                             const int32_t* graph_offsets, int64_t num_edges,
                             int num_edge_types, ggnn_stream_t stream);

/* T-step forward.  h0, hT: [b][v][h] fp32.  training != 0 keeps what the
 * backward needs inside ws (ws must have been sized with training != 0). */
int ggnn_forward(const ggnn_dims* d, const void* pack, const void* adj, void* ws,
                 int training, const float* h0, float* hT, ggnn_stream_t stream);

/* Backward of the last training forward on ws (same d, pack, adj).
 * dhT, dh0: [b][v][h] fp32.  Gradient outputs are OVERWRITTEN (not
 * accumulated), fp32, reference layouts; d_edge_biases may be NULL when
 * !(flags & GGNN_USE_EDGE_BIAS). */
int ggnn_backward(const ggnn_dims* d, const void* pack, const void* adj, void* ws,
                  const float* dhT, float* dh0,
                  float* d_edge_weights, float* d_edge_biases,
                  float* d_gates_kernel, float* d_gates_bias,
                  float* d_candidate_kernel, float* d_candidate_bias,
                  ggnn_stream_t stream);

/* The reference's optimizer step for the path's variables
 * (chem_tensorflow.py:494-503): every gradient scaled by grad_scale (1/N for
 * an N-rank data-parallel mean), clipped per tensor with tf.clip_by_norm
 * (g * clip_norm / max(||g||_2, clip_norm), params['clamp_gradient_norm']),
 * then one tf.compat.v1.train.AdamOptimizer update (learning_rate,
 * beta1 = 0.9, beta2 = 0.999, epsilon = 1e-8 in the reference):
 *   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ;
 *   p -= lr sqrt(1-b2^step)/(1-b1^step) m / (sqrt(v) + eps),  step >= 1.
 * scratch: device float[count * GGNN_ADAM_SCRATCH_PER_TENSOR].  Two
 * HBM-bound launches (per-tensor norms, then the update). */
#define GGNN_ADAM_SCRATCH_PER_TENSOR 256
typedef struct ggnn_adam_tensor {
  float* param;
  const float* grad;
  float* m;  /* first-moment slot, zero-initialised by the caller */
  float* v;  /* second-moment slot, zero-initialised by the caller */
  int64_t n;
  /* NULL, or a device float holding the squared norm clip_by_norm must use
   * instead of ||grad||^2 (before grad_scale): an embedding's gradient is an
   * IndexedSlices in the reference, whose norm runs over the per-lookup rows
   * (ggnn_embed_backward's lookup_sqnorm) */
  const float* sqnorm;
} ggnn_adam_tensor;
#define GGNN_ADAM_MAX_TENSORS 16
int ggnn_adam_step(const ggnn_adam_tensor* tensors, int count, float learning_rate,
                   float beta1, float beta2, float epsilon, float clip_norm,
                   int64_t step, float grad_scale, float* scratch, ggnn_stream_t stream);
/* The same with the step count read from device memory (a device int64,
 * >= 1) and the bias-corrected step size derived from it in-kernel: a step
 * captured in a hipGraph replays with whatever count the caller wrote there. */
int ggnn_adam_step_dev(const ggnn_adam_tensor* tensors, int count, float learning_rate,
                       float beta1, float beta2, float epsilon, float clip_norm,
                       const int64_t* step, float grad_scale, float* scratch,
                       ggnn_stream_t stream);

/* Materialise a dropout keep-mask (1 = kept, 0 = dropped) exactly as the
 * kernels apply it, for verification: kind 0 = edge-weight mask of timestep t
 * ([C][h][h] bytes), kind 1 = state mask of timestep t ([b][v][h] bytes). */
int ggnn_dropout_mask(const ggnn_dims* d, int kind, int t, uint8_t* mask, ggnn_stream_t stream);

/* ---- The callers either side of the path (btb task) ----
 *
 * Embedding front-end: get_initial_node_representation,
 * chem_tensorflow_dense.py:264-306.  Segment s copies row
 * word_inputs[g][i][column_s] of table_s into columns [o_s, o_s + width_s) of
 * h0[g][i] (o_s = sum of the earlier widths), times an embedding-dropout mask /
 * keep (tf.nn.dropout, keep = placeholders['emb_dropout_keep_prob']); columns
 * past the last segment are zero (the tf.pad to hidden_size, :303-305).  The
 * widths must sum to <= d->h (the reference's tf.pad fails otherwise).  Uses
 * d->b, d->v, d->h.  Rows outside [0, rows) give zero vectors (validate on the
 * host: tf.nn.embedding_lookup raises for them on the CPU). */
typedef struct ggnn_embed_segment {
  const float* table; /* [rows][width] fp32 */
  float* d_table;     /* its gradient (ggnn_embed_backward; overwritten) */
  int64_t rows;
  int32_t width;
  int32_t column;     /* column of word_inputs indexing this table */
} ggnn_embed_segment;
#define GGNN_EMBED_MAX_SEGMENTS 8
int ggnn_embed_forward(const ggnn_dims* d, const ggnn_embed_segment* segs, int nseg,
                       const int32_t* word_inputs, int ncols, float keep, uint64_t seed,
                       float* h0, ggnn_stream_t stream);
/* Gradients of the tables from dL/dh0 (+ dh0_add when not NULL: the two uses
 * of h0, the propagation input and the heads' concat), same keep and seed as
 * the forward.  lookup_sqnorm: device float[nseg] (overwritten), per TABLE the
 * sum of squares of its per-lookup gradient rows, i.e. the squared norm
 * tf.clip_by_norm takes of the reference's IndexedSlices gradient
 * (chem_tensorflow.py:498-500).  Segments sharing a d_table (btb: the loc
 * table, looked up by word_inputs columns 0 and 3) have ONE gradient whose
 * rows are both lookups' rows: their sum goes to the slot of the first such
 * segment, the later segments' slots are 0. */
int ggnn_embed_backward(const ggnn_dims* d, const ggnn_embed_segment* segs, int nseg,
                        const int32_t* word_inputs, int ncols, float keep, uint64_t seed,
                        const float* dh0, const float* dh0_add, float* lookup_sqnorm,
                        ggnn_stream_t stream);
/* The same, bit-reproducible (round 5): the lookups accumulate into a 64-bit
 * fixed-point copy of each table (2^-40 resolution, |element| < 2^23), whose
 * integer sums do not depend on the order the additions land in, and the
 * squared norms are summed in a fixed order.  ws: a device buffer of
 * ggnn_embed_workspace_bytes (which depends on the tables only, not on the
 * batch), ZERO-FILLED by the caller before its first use; every call leaves it
 * zero-filled again.  Segments sharing a d_table (which must then have one
 * shape) accumulate together, as in ggnn_embed_backward.  (ggnn_embed_backward
 * above adds fp32 atomics: its result can differ in the last bits from run to
 * run.) */
int ggnn_embed_workspace_bytes(const ggnn_embed_segment* segs, int nseg, size_t* bytes);
int ggnn_embed_backward_ws(const ggnn_dims* d, const ggnn_embed_segment* segs, int nseg,
                           const int32_t* word_inputs, int ncols, float keep, uint64_t seed,
                           const float* dh0, const float* dh0_add, float* lookup_sqnorm, void* ws,
                           ggnn_stream_t stream);
/* (ggnn_embed_backward_ws: a segment whose d_table is NULL gets no gradient
 * and a zero squared-norm slot.)
 * Segment `seg`'s gradient as the reference's IndexedSlices (values, indices;
 * chem_tensorflow.py:496-500): rows [cap][width] = the per-lookup gradient
 * rows (embedding dropout applied, keep / seed as the forward), ids [cap] =
 * the looked-up table rows (-1 out of range); rows b*v .. cap-1 are zero with
 * id -1.  The data-parallel step all-gathers these and accumulates the union
 * of every rank's lookups with ggnn_embed_backward_ws (keep 1, one segment,
 * v = 1) instead of all-reducing the dense table. */
int ggnn_embed_lookup_rows(const ggnn_dims* d, const ggnn_embed_segment* segs, int nseg, int seg,
                           const int32_t* word_inputs, int ncols, float keep, uint64_t seed,
                           const float* dh0, const float* dh0_add, float* rows, int32_t* ids,
                           int64_t cap, ggnn_stream_t stream);

/* Output heads: gated_regression for --pr btb, chem_tensorflow_dense.py:439-516
 * with MLP(2h, o, [], out_layer_dropout_keep_prob) (utils.py:40-84), and the
 * btb loss, chem_tensorflow.py:349-403:
 *   z = [h_T | h0] @ (W * mask / keep) + b      (rows = b*v nodes)
 *   probs = softmax(z) over o                    (computed_values [b, v*o])
 *   loss  = sum_rows -sum_o labels * log(probs) / target_num
 * target_num = sum(target_mask[task]) + SMALL_NUMBER (the caller's host
 * value; the _dev variants below read it from device memory).  One mask per
 * head per step (keep, seed; GGNN_SEED_DEVICE in d->flags: seed is the
 * address of a device uint64). */
typedef struct ggnn_output_head {
  const float* weight; /* MLP_W_layer0 [2h][o] */
  const float* bias;   /* MLP_b_layer0 [o] */
  int32_t o;           /* output width, 1..1024 */
  const float* labels; /* [b][v][o] targets, or NULL (no loss) */
  float* probs;        /* [b][v][o] out */
  float* d_weight;     /* [2h][o] (backward; overwritten) */
  float* d_bias;       /* [o]     (backward; overwritten) */
} ggnn_output_head;
#define GGNN_MAX_HEADS 4
int ggnn_heads_workspace_bytes(const ggnn_dims* d, const ggnn_output_head* heads, int nheads, size_t* bytes);
/* loss: device float[nheads], overwritten (per head; the reference's loss is
 * their sum).  ws is kept for ggnn_heads_backward. */
int ggnn_heads_forward(const ggnn_dims* d, const ggnn_output_head* heads, int nheads, const float* hT,
                       const float* h0, float keep, uint64_t seed, float target_num, float* loss,
                       void* ws, ggnn_stream_t stream);
/* d_loss: device float (dL/dloss, e.g. 1) or NULL for 1.  dhT, dh0: [b][v][h],
 * overwritten with the heads' contributions. */
int ggnn_heads_backward(const ggnn_dims* d, const ggnn_output_head* heads, int nheads, const float* hT,
                        const float* h0, float target_num, const float* d_loss, void* ws, float* dhT,
                        float* dh0, ggnn_stream_t stream);
/* The same two with target_num read from device memory (a device float > 0),
 * for hipGraph capture of a training step: identical results to passing that
 * value (the normaliser 1 / target_num and the power-of-two scale of dZ are
 * derived from it in the kernels). */
int ggnn_heads_forward_dev(const ggnn_dims* d, const ggnn_output_head* heads, int nheads, const float* hT,
                           const float* h0, float keep, uint64_t seed, const float* target_num, float* loss,
                           void* ws, ggnn_stream_t stream);
int ggnn_heads_backward_dev(const ggnn_dims* d, const ggnn_output_head* heads, int nheads, const float* hT,
                            const float* h0, const float* target_num, const float* d_loss, void* ws,
                            float* dhT, float* dh0, ggnn_stream_t stream);

/* Decoding of the two heads' probabilities on the device: the predicted head
 * and label of every node and the per-graph LAS / UAS counts, with the host
 * scorer's semantics (chem_tensorflow_dense.py:1054-1079 get_results_reshaped,
 * :106-131 adj_mat_to_target).  For graph g with n = n_nodes[g] (clamped to
 * [0, v]) and node i in 1..v-1:
 *   pred[g][i][0]  the first maximum over the o columns of probs_head[g][i][j]
 *                  * (j < n ? 1 : 0); pred[g][i][1] the first maximum over the
 *                  oe columns of probs_label[g][i][:].  -1 (skipped) when
 *                  i >= n, the maximum is 0, or the masked row holds a NaN.
 *   gold[g][i][0 / 1]  the first column of gold_head / gold_label [g][i][:]
 *                  equal to 1.0f, -1 when there is none (every row 1..v-1).
 *   counts[g] = { n_kept, las, uas, lab, regular }: the nodes with a gold head,
 *                  those of them whose predicted head and label / head / label
 *                  equal the gold ones, and regular = 1 when the four lists
 *                  (two without gold) skip the same nodes and no input of a
 *                  row i < n is NaN or +-inf (otherwise the reference's
 *                  position-wise list comparison differs from these counts:
 *                  score that graph on the host).
 * Row 0 of pred / gold is -1.  Values are zero-based column indices.  gold_head
 * and gold_label are given together or both NULL (then gold is not written and
 * the counts are 0 but for regular).  Needs v <= o and o, oe in 1..1024.
 * Stream-ordered, legal under stream capture, bit-reproducible. */
#define GGNN_DECODE_COUNTS 5 /* n_kept, las, uas, lab, regular */
int ggnn_heads_decode(const ggnn_dims* d, /* b, v used */
                      const float* probs_head, int32_t o, const float* probs_label, int32_t oe,
                      const float* gold_head,  /* [b][v][o]  or NULL */
                      const float* gold_label, /* [b][v][oe] or NULL */
                      const int32_t* n_nodes,  /* device [b] */
                      int32_t* pred,           /* device [b][v][2] out */
                      int32_t* gold,           /* device [b][v][2] out, or NULL */
                      int32_t* counts,         /* device [b][GGNN_DECODE_COUNTS] out */
                      ggnn_stream_t stream);

/* Tree-constrained decoding: a post-pass on ggnn_heads_decode's pred, on the
 * same stream.  scores are integer arc scores (heads.py tree_scores builds
 * them from the head probabilities).  For graph g with n = n_nodes[g] clamped
 * to [0, min(v, o)]:
 *   allowed arc   word i takes head j: 1 <= i < n, 0 <= j < n, j != i and
 *                 scores[g][i][j] != GGNN_TREE_FORBIDDEN; rows and columns >= n
 *                 are ignored whatever they hold.
 *   tree          every word 1..n-1 has one allowed head and following the
 *                 heads from any word reaches node 0; with single_root exactly
 *                 one word has head 0.
 *   status[g] = 0 pred[g][1..n-1][0] as passed in is a tree (or n < 2): nothing
 *                 of the graph is written and no contraction runs.
 *   status[g] = 2 no tree exists over the allowed arcs: nothing is written.
 *   status[g] = 1 pred[g][i][0], i in 1..n-1, is overwritten with a tree that
 *                 maximises the sum of scores[g][i][head_i] over all trees
 *                 (Chu-Liu/Edmonds; which of several optimal trees is chosen
 *                 is fixed by index order, the same from launch to launch).
 * The label column, row 0 and rows >= n are never written.  With gold and
 * counts (both, or both NULL) a repaired graph's counts[g][1] (las) and
 * counts[g][2] (uas) are recounted from the new heads by ggnn_heads_decode's
 * rule (rows with gold[g][i][0] >= 0); every other counter and every other
 * graph's counts stay.
 * Exactness: the arithmetic is 64-bit integer, and the result is exact for
 * EVERY int32 score other than GGNN_TREE_FORBIDDEN: a sum has at most 255
 * terms below 2^31, and single_root is a penalty of 2^42 per ROOT arc, which
 * exceeds any difference of two trees' totals (< 2^40); adjusted scores stay
 * within [-2^43, 2^31].  (tree_scores keeps S * v * (v + 1) < 2^30, S the
 * largest absolute score, so the totals also fit int32.)
 * Needs v <= o, v <= GGNN_TREE_MAXV and o <= 1024.  The kernel needs no
 * scratch: ggnn_tree_decode_workspace_bytes returns 0 and workspace may be
 * NULL.  Every loop of the kernel is bounded by a function of n.  Stream-
 * ordered, legal under stream capture, bit-reproducible; booked under the
 * heads kernel kind. */
#define GGNN_TREE_MAXV 256
#define GGNN_TREE_FORBIDDEN INT32_MIN
size_t ggnn_tree_decode_workspace_bytes(int32_t b, int32_t v);
int ggnn_tree_decode(const ggnn_dims* d,      /* b, v used */
                     const int32_t* scores,   /* device [b][v][o] */
                     int32_t o,
                     const int32_t* n_nodes,  /* device [b] */
                     int32_t single_root,     /* 0 / 1 */
                     int32_t* pred,           /* device [b][v][2], in/out: ggnn_heads_decode's */
                     const int32_t* gold,     /* device [b][v][2] or NULL */
                     int32_t* counts,         /* device [b][GGNN_DECODE_COUNTS] in/out, or NULL (with gold) */
                     int32_t* status,         /* device [b] out */
                     void* workspace, size_t workspace_bytes, ggnn_stream_t stream);

/* Projective decoding: the same post-pass with the best PROJECTIVE tree
 * (Eisner's O(n^3) span dynamic programme) in place of the maximum spanning
 * tree.  Arguments, allowed arcs, the tree rule and the clamping of n are
 * ggnn_tree_decode's; node 0 (ROOT) is the leftmost position.  A tree is
 * projective when no two of its arcs (i, head_i), (j, head_j) have endpoints
 * a < c < b < d, ROOT arcs included.
 *   status[g] = 0 pred[g][1..n-1][0] as passed in is a projective tree (with
 *                 single_root: with one ROOT child), or n < 2: nothing of the
 *                 graph is written and no table is filled.
 *   status[g] = 2 S * (n - 1) >= 2^30, S the largest absolute allowed score of
 *                 the graph (the range rule: below it every span total fits
 *                 int32, and the tables are int32), or no projective tree
 *                 exists over the allowed arcs: nothing is written.
 *   status[g] = 1 pred[g][i][0], i in 1..n-1, is overwritten with a projective
 *                 tree that maximises the sum of scores[g][i][head_i] over all
 *                 projective trees.  Among equal candidates the smallest split
 *                 point or ROOT child wins: the same bytes from launch to
 *                 launch.
 * single_root = 1 runs the tables over the words 1..n-1 and adds ROOT's one arc
 * at the end (no penalty constants); single_root = 0 runs them over 0..n-1
 * with node 0 never a dependent.  A span without a derivation holds -2^30
 * exactly, which no total can reach and which is never added to.
 * The label column, row 0 and rows >= n are never written.  gold / counts:
 * as ggnn_tree_decode (las and uas of a repaired graph recounted, every other
 * counter stays).
 * Storage: a graph with n <= GGNN_PROJ_LDS_MAXN keeps its four triangular
 * int32 tables (8 n (n + 1) bytes) in LDS, a larger one in `workspace`
 * (per graph; the tier follows the graph's n, not v).
 * ggnn_projective_decode_workspace_bytes(b, v) is 0 for v <=
 * GGNN_PROJ_LDS_MAXN and b * 8 * v * (v + 1) above; a smaller workspace is
 * rejected.  Needs v <= o, v <= GGNN_TREE_MAXV and o <= 1024.  One workgroup
 * per graph, no atomics, every loop bounded by a function of n.  Stream-
 * ordered, legal under stream capture, bit-reproducible; booked under the
 * heads kernel kind. */
#define GGNN_PROJ_LDS_MAXN 128
size_t ggnn_projective_decode_workspace_bytes(int32_t b, int32_t v);
int ggnn_projective_decode(const ggnn_dims* d,      /* b, v used */
                           const int32_t* scores,   /* device [b][v][o] */
                           int32_t o,
                           const int32_t* n_nodes,  /* device [b] */
                           int32_t single_root,     /* 0 / 1 */
                           int32_t* pred,           /* device [b][v][2], in/out: ggnn_heads_decode's */
                           const int32_t* gold,     /* device [b][v][2] or NULL */
                           int32_t* counts,         /* device [b][GGNN_DECODE_COUNTS] in/out, or NULL (with gold) */
                           int32_t* status,         /* device [b] out */
                           void* workspace, size_t workspace_bytes, ggnn_stream_t stream);

/* Projective arc marginals: the sum-product twin of ggnn_projective_decode.
 * The potential of "word i takes head j" in graph g is probs_head[g][i][j]
 * where the arc is allowed (finite, > 0, 1 <= i < n, 0 <= j < n, j != i; n
 * clamped as in ggnn_tree_decode); a projective dependency tree (ROOT
 * leftmost, no crossing arcs, single_root: exactly one ROOT child) weighs the
 * product of its words' potentials.
 *   logz[g]       ln of the sum of the weights of all such trees
 *   marg[g][i][j] the share of that sum held by the trees with the arc; 0 for
 *                 an arc that is not allowed, for row 0, rows >= n and columns
 *                 >= n.  Every word's row sums to 1, with single_root column 0
 *                 sums to 1 (both up to fp32 rounding).
 *   scores[g][i][j] (when not NULL) rint(marg * 2^20) for an allowed arc,
 *                 GGNN_TREE_FORBIDDEN otherwise: the integer scores whose
 *                 ggnn_projective_decode optimum is the minimum Bayes risk
 *                 tree (most expected-correct heads); 2^20 * 255 < 2^30, so
 *                 that call's range rule always holds.
 *   status[g] = 1 the above was written
 *   status[g] = 0 n < 2                       (logz = 0)
 *   status[g] = 2 no projective tree exists over the allowed arcs, or ln Z is
 *                 not finite                  (logz = -inf)
 * For status != 1 marg[g] is a copy of probs_head[g] (all v rows) and
 * scores[g] is GGNN_TREE_FORBIDDEN everywhere, so that everything downstream
 * behaves as the plain arg-max for that graph.  marg must not alias probs_head.
 * Inside and outside pass in log space, fp32, on ln p minus a per-word constant
 * (the row's largest ln p, then ln Z' / (n - 1) of a first inside pass on top:
 * the tables stay near 0; the marginals do not depend on the constants and
 * logz gets their sum back).  Storage: a
 * graph with n <= GGNN_MARG_LDS_MAXN keeps its seven triangular fp32 tables
 * (14 n (n + 1) bytes) in LDS, a larger one in `workspace` (per graph; the
 * tier follows the graph's n).  ggnn_projective_marginals_workspace_bytes(b,
 * v) is 0 for v <= GGNN_MARG_LDS_MAXN and b * 14 * v * (v + 1) above; a
 * smaller workspace is rejected.  Needs v <= o, v <= GGNN_TREE_MAXV, o <= 1024.
 * One workgroup per graph, no atomics, every loop bounded by a function of n,
 * every reduction in a fixed order.  Stream-ordered, allocation-free, legal
 * under stream capture, bit-reproducible; booked under the heads kernel kind.
 *
 * ggnn_arc_confidence: conf[g][i] = marg[g][i][pred[g][i][0]], 0 where the
 * predicted head is -1 (or >= o) or the row is 0 or >= n. */
#define GGNN_MARG_LDS_MAXN 107
size_t ggnn_projective_marginals_workspace_bytes(int32_t b, int32_t v);
int ggnn_projective_marginals(const ggnn_dims* d,        /* b, v used */
                              const float* probs_head,   /* device [b][v][o] */
                              int32_t o,
                              const int32_t* n_nodes,    /* device [b] */
                              int32_t single_root,       /* 0 / 1 */
                              float* marg,               /* device [b][v][o] out */
                              float* logz,               /* device [b] out */
                              int32_t* scores,           /* device [b][v][o] out, or NULL */
                              int32_t* status,           /* device [b] out */
                              void* workspace, size_t workspace_bytes, ggnn_stream_t stream);
int ggnn_arc_confidence(const ggnn_dims* d,              /* b, v used */
                        const float* marg,               /* device [b][v][o] */
                        int32_t o,
                        const int32_t* n_nodes,          /* device [b] */
                        const int32_t* pred,             /* device [b][v][2] */
                        float* conf,                     /* device [b][v] out */
                        ggnn_stream_t stream);

/* Arc marginals over ALL dependency trees (the matrix-tree theorem): what
 * ggnn_projective_marginals is to ggnn_projective_decode, this is to
 * ggnn_tree_decode.  Potentials, allowed arcs and the clamping of n are
 * ggnn_projective_marginals'; a dependency tree (single_root: exactly one ROOT
 * child) weighs the product of its words' potentials and may have crossing
 * arcs.  The outputs and their contract are ggnn_projective_marginals', word
 * for word: logz[g], marg[g][i][j] (0 for an arc that is not allowed, row 0,
 * rows and columns >= n; clamped to [0, 1]), scores[g][i][j] (when not NULL)
 * rint(marg * 2^20) on allowed arcs and GGNN_TREE_FORBIDDEN elsewhere --
 * ggnn_tree_decode, exact for every int32 score, gives their minimum Bayes
 * risk tree --, status[g] = 1 written, 0 n < 2 (logz = 0), 2 no tree (logz =
 * -inf); for status != 1 marg[g] is a copy of probs_head[g] and scores[g] is
 * GGNN_TREE_FORBIDDEN everywhere.  marg must not alias probs_head.
 * Every word's row is divided by its sum c[i] (scaled by the power of two of
 * its largest entry first; logz gets sum ln c[i] back).  With w / r the
 * normalised potentials of a word head / of ROOT, the (n-1) x (n-1) matrix
 * over the words is A[h][d] = -w(d, h), A[d][d] = r(d) + sum_h w(d, h);
 * single_root (Koo et al. 2007): A[d][d] = sum_h w(d, h) and the first word's
 * row holds r(.).  Z = det A, the marginals come from the inverse, computed in
 * fp32 by in-place Gauss-Jordan elimination with partial pivoting (the largest
 * absolute value of the column, the smallest row among equals); ln Z is summed
 * in double.  Whether a tree exists is decided on the allowed arcs by
 * reachability (multi-root: ROOT reaches every word head -> dependent;
 * single_root: a word with an allowed ROOT arc reaches every word), never on
 * a pivot; status 2 is also the answer when a pivot is 0 or not finite, the
 * determinant is not positive or ln Z is not finite.  A marginal is off by
 * about n * cond_1(A) * 2^-24.
 * Storage: a graph with n <= GGNN_LAPL_LDS_MAXN keeps its matrix in LDS
 * ((n-1) rows of (n-1)|1 floats: 157,608 B at 199, 163,264 B of the CU's
 * 163,840 with the row sums, the pivot record and the permutation; the
 * reachability bits, 16 KiB, lie in the matrix before it is built), a larger
 * one in `workspace` (per graph; the tier follows the graph's n).
 * ggnn_tree_marginals_workspace_bytes(b, v) is 0 for v <= GGNN_LAPL_LDS_MAXN
 * and b * 4 * (v-1) * ((v-1)|1) above; a smaller workspace is rejected.  Needs
 * v <= o, v <= GGNN_TREE_MAXV, o <= 1024.  One workgroup per graph, no
 * atomics, every loop bounded by a function of n, every reduction in a fixed
 * order.  Stream-ordered, allocation-free, legal under stream capture,
 * bit-reproducible; booked under the heads kernel kind.  ggnn_arc_confidence
 * gathers the returned heads' marginals from marg as it is. */
#define GGNN_LAPL_LDS_MAXN 199
size_t ggnn_tree_marginals_workspace_bytes(int32_t b, int32_t v);
int ggnn_tree_marginals(const ggnn_dims* d,        /* b, v used */
                        const float* probs_head,   /* device [b][v][o] */
                        int32_t o,
                        const int32_t* n_nodes,    /* device [b] */
                        int32_t single_root,       /* 0 / 1 */
                        float* marg,               /* device [b][v][o] out */
                        float* logz,               /* device [b] out */
                        int32_t* scores,           /* device [b][v][o] out, or NULL */
                        int32_t* status,           /* device [b] out */
                        void* workspace, size_t workspace_bytes, ggnn_stream_t stream);

/* The tree-structured training loss (Koo et al. 2007): the negative
 * log-likelihood of the gold tree under the distribution that
 * ggnn_tree_marginals (family 0: all dependency trees) or
 * ggnn_projective_marginals (family 1: projective trees) define.  For one graph
 *   L = -sum_d ln p[d][gold_d] + ln Z,   dL/dz[d][k] = marg[d][k] - y[d][k]
 * (z the head logits, p their softmax, y = gold_head).  The first term is the
 * cross-entropy ggnn_heads_forward has already put into the loss; this call,
 * after it on the same stream, adds the second and leaves in marg what
 * ggnn_heads_backward takes in head 0's `probs` place (its dZ = g * (probs *
 * sum(y) - y) is then g * (marg - y) on every row with one gold head and 0 on
 * row 0 and the padding rows).
 * A graph is ELIGIBLE when, with n = n_nodes[g] clamped as in ggnn_tree_decode,
 * n >= 2 and
 *   every row 1..n-1 of gold_head[g] holds exactly one 1.0f and zeros otherwise,
 *   that column is an allowed arc of the marginals (< n, not the word itself,
 *   its potential finite and > 0),
 *   row 0 and the rows >= n are all zero,
 *   following the heads from any word reaches node 0,
 *   with single_root exactly one word takes column 0, and
 *   with family 1 no two arcs cross (ROOT leftmost),
 * i.e. when the gold tree has a probability under the distribution.  Three
 * launches: the eligibility kernel writes n_eff[g] = n or 0 into the workspace;
 * the family's marginal kernel runs unchanged on n_eff (scores = NULL) and
 * writes marg, logz and status by its own contract, so that a graph that is
 * not eligible (status 0) or has no finite ln Z (status 2) keeps marg[g] = a
 * byte copy of probs_head[g], i.e. the plain cross-entropy and its gradient;
 * the last sets used[g] = (status[g] == 1) and
 *   loss_inout[0] += (sum over the used graphs of logz[g]) / target_num,
 * the sum taken in double in a fixed order.  target_num: as ggnn_heads_forward
 * (the _dev form reads a device float > 0; the two give the same bits).
 * ggnn_tree_loss_workspace_bytes(b, v, family) = b int32 rounded up to 256
 * bytes + the family's marginals workspace (0 up to GGNN_LAPL_LDS_MAXN /
 * GGNN_MARG_LDS_MAXN nodes); a smaller workspace is rejected.  Needs v <= o,
 * v <= GGNN_TREE_MAXV, o <= 1024; marg must not alias probs_head.  No atomics,
 * every loop bounded by a function of n.  Stream-ordered, allocation-free,
 * legal under stream capture, bit-reproducible; booked under the heads kernel
 * kind. */
size_t ggnn_tree_loss_workspace_bytes(int32_t b, int32_t v, int32_t family);
int ggnn_tree_loss(const ggnn_dims* d,        /* b, v used */
                   const float* probs_head,   /* device [b][v][o] */
                   int32_t o,
                   const float* gold_head,    /* device [b][v][o] */
                   const int32_t* n_nodes,    /* device [b] */
                   int32_t family,            /* 0 all dependency trees, 1 projective */
                   int32_t single_root,       /* 0 / 1 */
                   float target_num,
                   float* marg,               /* device [b][v][o] out */
                   float* logz,               /* device [b] out */
                   int32_t* status,           /* device [b] out */
                   int32_t* used,             /* device [b] out */
                   float* loss_inout,         /* device float, added to */
                   void* workspace, size_t workspace_bytes, ggnn_stream_t stream);
int ggnn_tree_loss_dev(const ggnn_dims* d, const float* probs_head, int32_t o, const float* gold_head,
                       const int32_t* n_nodes, int32_t family, int32_t single_root,
                       const float* target_num, /* device float */
                       float* marg, float* logz, int32_t* status, int32_t* used, float* loss_inout,
                       void* workspace, size_t workspace_bytes, ggnn_stream_t stream);

/* The max-margin training loss: the structured hinge over cost-augmented
 * decoding (Taskar et al. 2004; MSTParser; Kiperwasser & Goldberg 2016), the
 * max-product twin of ggnn_tree_loss.  For one graph, with s the integer scores
 * rint(log2 p * 2^k) of the head probabilities (floor -150 * 2^k, k the largest
 * k <= 16 with 150 * 2^k * v * (v + 1) <= 2^30, GGNN_TREE_FORBIDDEN where the
 * arc is not allowed), y the gold heads and C = rint(cost * 2^k / ln 2),
 *   T* = the maximum tree of s'[d][j] = s[d][j] + C [j != y_d] in the family
 *        (ggnn_tree_decode, family 0; ggnn_projective_decode, family 1),
 *   l  = sum over the words with T*_d != y_d of ln p[d][T*_d] - ln p[d][y_d] + cost
 *        (in double, from the float32 p),
 *   L  = max(0, l),   dL/dz[d][k] = onehot(T*)[d][k] - y[d][k] where l > 0, else 0
 * (z the head logits: every tree has one head per word, so the rows' logsumexp
 * cancels between two trees).  l falls short of the true maximum over the
 * family by at most 1.5 (n - 1) ln 2 * 2^-k, the resolution of the scores.
 * Eligibility is ggnn_tree_loss's.  A graph is USED when it is eligible and the
 * decoder's status is 1; for a used graph L replaces the cross-entropy that
 * ggnn_heads_forward has put into the loss, any other graph keeps it.  The call
 * runs after ggnn_heads_forward on the same stream and leaves in marg what
 * ggnn_heads_backward takes in head 0's `probs` place:
 *   used, l > 0:   onehot(T*) on the rows 1..n-1, zeros elsewhere;
 *   used, l <= 0:  a copy of gold_head[g] (dZ = 0);
 *   not used:      a byte copy of probs_head[g].
 * heads[g][i] = T*_i for the words of a used graph, -1 on node 0, the padding
 * and every other graph; value[g] = L (0 where not used); hamming[g] = the
 * number of words with T*_d != y_d (0 where not used); status[g] = the
 * decoder's (0 for a graph that is not eligible); used[g] = 0 / 1; and
 *   loss_inout[0] += (sum over the used graphs of L + sum_d ln p[d][y_d]) / target_num,
 * the per-graph values and the sum in double in a fixed order.  Five launches:
 * the eligibility kernel of ggnn_tree_loss, the scores, the family's decoder
 * unchanged (every head of its pred at -1, so it always solves), the per-graph
 * fold, the sum.  Needs 0 <= cost <= 64 (finite; then |s'| <= 150 * 2^k, the
 * range the shift guarantees), v <= o, v <= GGNN_TREE_MAXV, o <= 1024; marg
 * must not alias probs_head.  ggnn_margin_loss_workspace_bytes(b, v, o,
 * family): n_eff, the per-graph doubles, the gold heads, pred and s' (each
 * rounded up to 256 bytes) + the decoder's workspace; a smaller workspace is
 * rejected.  target_num: as ggnn_tree_loss (the _dev form gives the same
 * bits).  No atomics, no host synchronisation, no allocation; stream-ordered,
 * legal under stream capture, bit-reproducible; booked under the heads kernel
 * kind. */
size_t ggnn_margin_loss_workspace_bytes(int32_t b, int32_t v, int32_t o, int32_t family);
int ggnn_margin_loss(const ggnn_dims* d,        /* b, v used */
                     const float* probs_head,   /* device [b][v][o] */
                     int32_t o,
                     const float* gold_head,    /* device [b][v][o] */
                     const int32_t* n_nodes,    /* device [b] */
                     int32_t family,            /* 0 all dependency trees, 1 projective */
                     int32_t single_root,       /* 0 / 1 */
                     float cost,                /* the margin per wrong head, 0..64 */
                     float target_num,
                     float* marg,               /* device [b][v][o] out */
                     int32_t* heads,            /* device [b][v] out */
                     float* value,              /* device [b] out */
                     int32_t* hamming,          /* device [b] out */
                     int32_t* status,           /* device [b] out */
                     int32_t* used,             /* device [b] out */
                     float* loss_inout,         /* device float, added to */
                     void* workspace, size_t workspace_bytes, ggnn_stream_t stream);
int ggnn_margin_loss_dev(const ggnn_dims* d, const float* probs_head, int32_t o, const float* gold_head,
                         const int32_t* n_nodes, int32_t family, int32_t single_root, float cost,
                         const float* target_num, /* device float */
                         float* marg, int32_t* heads, float* value, int32_t* hamming, int32_t* status,
                         int32_t* used, float* loss_inout, void* workspace, size_t workspace_bytes,
                         ggnn_stream_t stream);

/* Dependency trees drawn from the distribution that ggnn_tree_marginals
 * describes (weight of a tree: the product of its words' head probabilities,
 * crossing arcs included; single_root: exactly one ROOT child): num_samples = K
 * trees per graph.  Potentials, allowed arcs, the clamping of n and the
 * normalised w(d, h) / r(d) are ggnn_tree_marginals'.  marg, logz and
 * marg_status are that call's outputs for the same probs_head, n_nodes and
 * single_root (marg is read with single_root only and may be NULL without).
 * Conditional (ancestral) sampling on the matrix-tree inverse, no random walk:
 * B = inverse of the multi-root matrix A[h][d] = -w(d, h), A[d][d] = r(d) +
 * sum_h w(d, h), by ggnn_tree_marginals' pivoted Gauss-Jordan elimination.
 * single_root first draws the one ROOT child rho with masses marg[g][d][0] over
 * the words that have an allowed ROOT arc and reach every word (the
 * reachability rows of the feasibility test: a structural mask), then builds A
 * with r'(d) = [d == rho] and word rho's word potentials zeroed; rho has no
 * step of its own.  The words d = 1..n-1 are walked in ascending order:
 *   masses  q_0 = r'(d) B[d][d], q_h = w(d, h) (B[d][d] - B[d][h]), clamped at
 *           0, 0 for an arc that is not allowed and for an h whose chain of
 *           already fixed heads ends in d (it would close a cycle): a returned
 *           sample is a tree by construction;
 *   draw    u = (x >> 8) * 2^-24, x the first word of Philox4x32-10 at counter
 *           (d, s, g, 0x40000000) (d = 0: the ROOT child's draw; s the sample,
 *           g the graph) with the 64-bit seed as key (low word first).  With
 *           inclusive prefix sums c_j in ascending column order and S the
 *           last, the head is the smallest j with q_j > 0 and c_j > u * S, the
 *           largest j with q_j > 0 if rounding leaves none;
 *   update  cvec = B[:, d] - e_d - [h* > 0] B[:, h*], den = B[d][d] - [h* > 0]
 *           B[d][h*], B <- B - cvec (x) B[d, :] / den (Sherman-Morrison).
 * Outputs: heads[g][s][i] the head of word i, -1 on row 0, rows >= n and where
 * status != 1; log_prob[g][s] = sum_d ln probs_head[d][head_d] - logz[g],
 * summed in double in word order, -inf where status != 1; status[g][s] = 1
 * drawn, marg_status[g] (0 or 2) where that is not 1, 2 on a numerical dead
 * end (S not > 0, den not finite and positive).  Sample s of graph g depends
 * on (seed, g, s) alone, not on num_samples.
 * Storage: a graph with n <= GGNN_SAMPLE_LDS_MAXN keeps its matrix in LDS
 * (ggnn_tree_marginals' budget: the side arrays lie in fields that are dead
 * after the inversion), a larger one in `workspace`, per (graph, sample); the
 * tier follows the graph's n.  ggnn_tree_sample_workspace_bytes(b, v, K) is 0
 * for v <= GGNN_SAMPLE_LDS_MAXN and b * K * 4 * (v-1) * ((v-1)|1) above; a
 * smaller workspace is rejected.  Needs v <= o, v <= GGNN_TREE_MAXV, o <= 1024,
 * 1 <= num_samples <= GGNN_SAMPLE_MAX.  One workgroup per (graph, sample), no
 * atomics, nothing between workgroups, every loop bounded by a function of n,
 * every reduction and scan in a fixed order.  Stream-ordered, allocation-free,
 * legal under stream capture, bit-reproducible; booked under the heads kernel
 * kind. */
#define GGNN_SAMPLE_LDS_MAXN 199
#define GGNN_SAMPLE_MAX 4096
size_t ggnn_tree_sample_workspace_bytes(int32_t b, int32_t v, int32_t num_samples);
int ggnn_tree_sample(const ggnn_dims* d,           /* b, v used */
                     const float* probs_head,      /* device [b][v][o] */
                     int32_t o,
                     const int32_t* n_nodes,       /* device [b] */
                     int32_t single_root,          /* 0 / 1 */
                     const float* marg,            /* device [b][v][o], or NULL without single_root */
                     const float* logz,            /* device [b] */
                     const int32_t* marg_status,   /* device [b] */
                     int32_t num_samples, uint64_t seed,
                     int32_t* heads,               /* device [b][K][v] out */
                     float* log_prob,              /* device [b][K] out */
                     int32_t* status,              /* device [b][K] out */
                     void* workspace, size_t workspace_bytes, ggnn_stream_t stream);

/* Projective dependency trees drawn from the distribution that
 * ggnn_projective_marginals describes (weight of a tree: the product of its
 * words' head probabilities, over the trees without crossing arcs, ROOT
 * leftmost; single_root: exactly one ROOT child): num_samples = K trees per
 * graph.  Self-contained: no prior marginals call is needed.  Potentials,
 * allowed arcs, the clamping of n, the positions p = 0..m-1, the tables CR, CL,
 * IR, IL, their two inside passes and ln Z are ggnn_projective_marginals'.  One
 * inside pass serves every sample of a graph; a sample expands items top-down.
 * An item (kind, s, t) stands for one table entry; its terms, in ascending r:
 *   0  ROOT's child (single_root; s = t = 0)
 *                      r = 0..m-1: CL[0][r] + CR[r][m-1] + psi(r+1 takes ROOT)
 *                      children CL[0][r], CR[r][m-1]; head of word r+1 = 0
 *   1  CR[s][t], s < t r = s+1..t: IR[s][r] + CR[r][t]     children: those two
 *   2  CL[s][t], s < t r = s..t-1: CL[s][r] + IL[r][t]     children: those two
 *   3  IR[s][t]        r = s..t-1: CR[s][r] + CL[r+1][t]   children: those two;
 *                      node lo+t takes lo+s
 *   4  IL[s][t]        as kind 3; node lo+s takes lo+t
 * The start item is kind 0, CR[0][m-1] without single_root; items of kinds 1
 * and 2 with s = t are leaves; the order in which pending items are expanded
 * does not matter.  The draw of an item:
 *   masses  q_r = expf(term_r - M), M the largest term, 0 for a -inf term;
 *   draw    u = (x >> 8) * 2^-24, x the first word of Philox4x32-10 at counter
 *           (kind << 16 | s << 8 | t, sample, graph, 0x50000000) with the
 *           64-bit seed as key (low word first).  With inclusive prefix sums
 *           c_r in ascending r and S the last, the chosen term is the smallest
 *           r with q_r > 0 and c_r > u * S, the largest r with q_r > 0 if
 *           rounding leaves none.
 * A chosen term is finite, so both children have a derivation: a returned
 * sample is a projective tree over allowed arcs with the right ROOT count by
 * construction; S not > 0 is the only dead end.
 * Outputs: heads[g][s][i] the head of word i, -1 on row 0, rows >= n and where
 * status != 1; log_prob[g][s] = sum_d ln probs_head[d][head_d] - ln Z (the
 * terms logf in fp32, summed in double in word order), -inf where status != 1;
 * status[g][s] = 1 drawn, 0 n < 2, 2 no projective tree, ln Z not finite or a
 * dead end (the graphs of ggnn_projective_marginals' status 0 / 2); logz[g]
 * (when not NULL) as ggnn_projective_marginals defines it: 0 for status 0,
 * -inf for no projective tree.  Sample s of graph g depends on (seed, g, s)
 * alone, not on num_samples.
 * Storage: four fp32 triangular tables, 8 m (m + 1) bytes.  A graph with n <=
 * GGNN_PROJ_SAMPLE_LDS_MAXN keeps them in LDS (132,096 B at 128, 141,320 B
 * with c[], the four waves' item stacks and head rows), a larger one in
 * `workspace`, per (graph, chunk of GGNN_PROJ_SAMPLE_CHUNK consecutive
 * samples); the tier follows the graph's n.  At most m - 1 items are pending
 * at once (their spans lie side by side), so a stack of GGNN_TREE_MAXV entries
 * cannot overflow.  ggnn_projective_sample_workspace_bytes(b, v, K) is 0 for v
 * <= GGNN_PROJ_SAMPLE_LDS_MAXN and b * ceil(K / GGNN_PROJ_SAMPLE_CHUNK) * 8 * v
 * * (v + 1) above; a smaller workspace is rejected.  Needs v <= o, v <=
 * GGNN_TREE_MAXV, o <= 1024, 1 <= num_samples <= GGNN_SAMPLE_MAX.  One
 * workgroup per (graph, chunk): it fills the tables, then each of its four
 * waves walks the chunk's samples wave, wave + 4, ...  No atomics, nothing
 * between workgroups, every loop bounded by a function of n, every reduction
 * and scan in a fixed order.  Stream-ordered, allocation-free, legal under
 * stream capture, bit-reproducible; booked under the heads kernel kind. */
#define GGNN_PROJ_SAMPLE_LDS_MAXN 128
#define GGNN_PROJ_SAMPLE_CHUNK 16
size_t ggnn_projective_sample_workspace_bytes(int32_t b, int32_t v, int32_t num_samples);
int ggnn_projective_sample(const ggnn_dims* d,           /* b, v used */
                           const float* probs_head,      /* device [b][v][o] */
                           int32_t o,
                           const int32_t* n_nodes,       /* device [b] */
                           int32_t single_root,          /* 0 / 1 */
                           int32_t num_samples, uint64_t seed,
                           int32_t* heads,               /* device [b][K][v] out */
                           float* log_prob,              /* device [b][K] out */
                           int32_t* status,              /* device [b][K] out */
                           float* logz,                  /* device [b] out, or NULL */
                           void* workspace, size_t workspace_bytes, ggnn_stream_t stream);

/* The K best projective dependency trees of the integer head scores, in order
 * (Huang & Chiang 2005 on Eisner's tables): what ggnn_projective_decode returns
 * once, this returns K times.  scores, allowed arcs, the clamping of n, the
 * positions p = 0..m-1 (lo / m), the four span kinds, the -2^30 sentinel and
 * the range rule are ggnn_projective_decode's; a graph with S * (n - 1) >= 2^30
 * gets status 2.  There is no pred and no fast path: the tables are always
 * filled.  Every item holds a LIST of up to K entries.  IR and IL of a span
 * differ by the arc's score alone and share one base list BS:
 *   BS[s][t]  candidates (r, i, j), s <= r < t:  CR[s][r][i] + CL[r+1][t][j]
 *   CR[s][t]  candidates (r, i, j), s < r <= t:  BS[s][r][i] + score(r takes s) + CR[r][t][j]
 *   CL[s][t]  candidates (r, i, j), s <= r < t:  CL[s][r][i] + BS[r][t][j] + score(r takes t)
 *   final     single_root: (p, i, j): CL[0][p][i] + CR[p][m-1][j] + score(p+1
 *             takes ROOT); otherwise CR[0][m-1]'s list
 * (i, j: ranks in the first / second entry's list).  A candidate exists when
 * both entries exist and the arc is allowed; a list is the first K candidates
 * in the total order: larger total first, then the smaller split r (p), then
 * the smaller i, then the smaller j.  The result is a function of the inputs
 * alone.  Every projective tree has exactly one derivation, so the final list
 * holds min(K, number of projective trees) distinct trees; rank 0 is
 * ggnn_projective_decode's tree, ties included; the list for K is a prefix of
 * the list for any larger K.  Every entry stores its (split, i, j); the tree of
 * a rank is read back from those, never found again by value.
 * Outputs: heads[g][k][i] the head of word i in the tree of rank k, -1 on node
 * 0, rows >= n and ranks >= count[g]; totals[g][k] = sum_i scores[i][head_i],
 * GGNN_TREE_FORBIDDEN on ranks >= count[g]; count[g] in 0..K; status[g] = 0 n <
 * 2 (count 0), 1 count >= 1, 2 the range rule is violated or no projective
 * tree exists (count 0).
 * Storage: per span 6 K + 2 int32 (three value lists, three back-pointer
 * lists, two arc scores), m (m + 1) / 2 spans.  A graph with n <=
 * ggnn_projective_kbest_lds_maxn(K) -- the largest n with n (n + 1) / 2 * (6 K
 * + 2) <= 38400 ints: 97 at K = 1, 73 at 2, 27 at 16 -- keeps them in LDS
 * (153,600 B; 161,940 B with the four waves' item stacks and head rows and the
 * final list), a larger one in `workspace`, per graph; the tier follows the
 * graph's n.  ggnn_projective_kbest_workspace_bytes(b, v, K) is 0 for v <=
 * ggnn_projective_kbest_lds_maxn(K) and b * 2 * v * (v + 1) * (6 K + 2) above;
 * a smaller workspace is rejected before any launch.  Fewer than m items are
 * pending in a walk-back at once, so a stack of GGNN_TREE_MAXV entries cannot
 * overflow; an overflow or a walk of more than 2 m - 1 items would be status
 * 2.  Needs v <= o, v <= GGNN_TREE_MAXV, o <= 1024, 1 <= K <= GGNN_KBEST_MAX.
 * One workgroup per graph: it fills the lists length by length (K rounds of
 * "next in order" per item, a span's splits spread over a lane group), then
 * each of its four waves reads back the ranks wave, wave + 4, ...  No atomics,
 * nothing between workgroups, every loop bounded by a function of n and K.
 * Stream-ordered, allocation-free, legal under stream capture,
 * bit-reproducible; booked under the heads kernel kind. */
#define GGNN_KBEST_MAX 16
int32_t ggnn_projective_kbest_lds_maxn(int32_t K);
size_t ggnn_projective_kbest_workspace_bytes(int32_t b, int32_t v, int32_t K);
int ggnn_projective_kbest(const ggnn_dims* d,           /* b, v used */
                          const int32_t* scores,        /* device [b][v][o] */
                          int32_t o,
                          const int32_t* n_nodes,       /* device [b] */
                          int32_t single_root,          /* 0 / 1 */
                          int32_t K,
                          int32_t* heads,               /* device [b][K][v] out */
                          int32_t* totals,              /* device [b][K] out */
                          int32_t* count,               /* device [b] out */
                          int32_t* status,              /* device [b] out */
                          void* workspace, size_t workspace_bytes, ggnn_stream_t stream);

/* The K best trees over ALL dependency trees (arcs may cross) of every graph,
 * in order: ggnn_projective_kbest's twin in the family of ggnn_tree_decode.
 * Arguments, argument order, limits, the range rule and the outputs' fills are
 * ggnn_projective_kbest's: heads[g][k][i] the head of word i in the tree of
 * rank k, -1 on node 0, rows >= n and ranks >= count[g]; totals[g][k] = sum_i
 * scores[i][head_i], GGNN_TREE_FORBIDDEN on ranks >= count[g]; count[g] in
 * 0..K = min(K, number of trees); status[g] = 0 n < 2 (count 0), 1 count >= 1,
 * 2 the range rule is violated or no tree exists (count 0).  single_root: every
 * tree has one ROOT child.
 * Lawler's partitioning over ggnn_tree_decode's Chu-Liu/Edmonds solver.  A
 * subproblem = a partial head assignment and a list of excluded arcs; its best
 * tree is the maximum arborescence of the scores with a fixed word's row
 * forbidden except at its head and every excluded arc forbidden.  Rank 0 is
 * the unconstrained optimum: ggnn_tree_decode's tree when that pass runs, ties
 * included.  The tree h that becomes rank r leaves one child per word w its
 * subproblem leaves free, in increasing w: the free words below w fixed to
 * their heads in h, (w, h[w]) excluded on top of the inherited exclusions (at
 * most K - 1 on a chain).  Every solved child's total goes to a pool; rank r +
 * 1 is the pool's first entry by: larger total, then smaller parent rank, then
 * smaller word.  The children partition their parent's subproblem without h,
 * so the list holds distinct trees; nothing depends on K, so the list for K is
 * a prefix of the list for any larger K.
 * 2 K - 1 stream-ordered launches, no host synchronisation: take(0), then
 * solve(r - 1) (grid b * (v - 1): child (r - 1, w) of graph g, one workgroup
 * each; those of absent ranks, of rows >= n and of fixed words leave at once)
 * and take(r) (grid b: the pool's first entry, its child solved again for the
 * heads, which are never stored) for r = 1 .. K - 1; K = 1 launches take(0)
 * alone.  At most (K - 1)(n - 1) + K contractions per graph.
 * Storage: ggnn_tree_kbest_workspace_bytes(b, v, K) = b * 4 * (K * (2 v + 16)
 * + 16) bytes (0 for b < 1, v < 1 or K outside 1..GGNN_KBEST_MAX): per graph 16
 * int32 (the ranks so far), the pool K * v and per rank v + 16 (fix[v], 15
 * exclusions, their number); nothing of size v^2.  A smaller workspace is
 * rejected before any launch.  Needs v <= o, v <= GGNN_TREE_MAXV, o <= 1024, 1
 * <= K <= GGNN_KBEST_MAX, b * (v - 1) < 2^31.  Workgroups of 256 threads, 30.2
 * KiB of LDS each.  No atomics, nothing between the workgroups of a launch,
 * every loop bounded by a function of n and K, every tie by index order.
 * Allocation-free, legal under stream capture, bit-reproducible; booked under
 * the heads kernel kind. */
size_t ggnn_tree_kbest_workspace_bytes(int32_t b, int32_t v, int32_t K);
int ggnn_tree_kbest(const ggnn_dims* d,                 /* b, v used */
                    const int32_t* scores,              /* device [b][v][o] */
                    int32_t o,
                    const int32_t* n_nodes,             /* device [b] */
                    int32_t single_root,                /* 0 / 1 */
                    int32_t K,
                    int32_t* heads,                     /* device [b][K][v] out */
                    int32_t* totals,                    /* device [b][K] out */
                    int32_t* count,                     /* device [b] out */
                    int32_t* status,                    /* device [b] out */
                    void* workspace, size_t workspace_bytes, ggnn_stream_t stream);

/* Optional per-kernel timing (HIP events around every launch of the library
 * on the launch's stream), used by bench.py for the roofline.  Not for use
 * under graph capture.  total_ms / launches: arrays of GGNN_NUM_KERNEL_KINDS. */
#define GGNN_NUM_KERNEL_KINDS 11
const char* ggnn_kernel_kind_name(int kind);
int ggnn_profile_begin(int max_launches);
int ggnn_profile_end(double* total_ms, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* GGNN_H */
