/*
 * gw_amd.h - C ABI of libgw_amd.so: the MI355X (gfx950) implementation of the message-passing hot path of
 * openclimatefix/graph_weather's GraphWeatherForecaster.
 *
 * The reference has no FFI: its boundary is the Python nn.Module API.  Each entry point below names the
 * reference statements it replaces (paths relative to the reference tree).  All functions
 *   - take plain device pointers + sizes + a hipStream_t passed as void* (no torch types),
 *   - never allocate, free or synchronise; they enqueue kernels on `stream` and return,
 *   - return 0 on success, a negative GW_E_* code otherwise (message via gw_last_error()).
 *
 * Data layout: activations row-major fp32 [rows, ld]; "tables" are [batch, rows_per_batch, ld] stacked along
 * rows (rows_per_batch == 0 means the table is shared by every batch element).  Edge lists are destination-
 * sorted int32 arrays shared by all batch elements ("shared graph" semantics, the reference's own
 * efficient_batching equivalence: tests/models/layers/test_efficient_batching.py:145).
 *
 * Weights are consumed in a packed MFMA-operand order produced by gw_pack_linear() from the reference's
 * nn.Linear layout ([out_features, in_features] row-major).
 */
#ifndef GW_AMD_H
#define GW_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GW_OK 0
#define GW_E_BADARG (-1)
#define GW_E_UNSUPPORTED (-2)
#define GW_E_LAUNCH (-3)

#define GW_ABI_VERSION 19

/* dtype of the packed weight stream of an MLP (activations in HBM, accumulation, LayerNorm, residuals and segment
 * sums are always fp32). GW_DTYPE_BF16: matrix products on v_mfma_f32_16x16x32_bf16, operands rounded to bf16 (RNE)
 * in registers - BASELINE.json configs[2]. */
#define GW_DTYPE_F32 0
#define GW_DTYPE_BF16 1
/* GW_DTYPE_BF16X3 (v16): split-operand products.  Both operands of every Linear (graph_net_block.py:45-61: fp32 in the reference)
 * are carried as a pair of bf16 values, v = hi + lo with hi = bf16(v), lo = bf16(v - hi) (16 significant bits, fp32 exponent
 * range), and x . w is evaluated as x_hi . w_hi + x_hi . w_lo + x_lo . w_hi on v_mfma_f32_16x16x32_bf16 with fp32 accumulation
 * (csrc/gw_split.hip): ~1e-5 per product - inside BASELINE.json's 1e-3 - at 3 bf16 MFMAs per product.  Streams from
 * gw_pack_linear_bf16x3 (4 bytes per weight).  Every table this mode reads or writes is fp32 rows (GW_LAYOUT_ROWS_F32): none of
 * the bf16 mode's 16-bit formats (edge tiles, fp16 product rows, bf16 K-order aggregates, segment-aligned tiles) applies.
 * Trains: the forward entry points accept gw_activation_save with these weights (fp32 saves: relu outputs of every Linear,
 * pre-LayerNorm rows), the backward's masked input-gradient products run through gw_mlp_ln_chain_backward /
 * gw_mlp_chain_backward_bf16x3 (gw_project_forward with relu_mask for single products) on transposed split packs and its
 * weight-gradient GEMMs through gw_gemm_f32 with GW_GEMM_TN_BF16X3; only GW_DTYPE_BF16 is inference-only.
 * Mesh-sized node updates (gw_node_update_forward with at most 12 288 rows, fp32 and bf16x3 weights alike) run on the row-split
 * kernels of csrc/gw_noders.hip - same arguments, bitwise the rows of the 64-column kernels. */
#define GW_DTYPE_BF16X3 2

/* Memory layout of a per-edge table handed to / produced by gw_edge_update_forward.
 * GW_LAYOUT_ROWS_F32: row-major fp32 rows (the reference's layout, graph_net_block.py:279-301 carries [E, D] tensors).
 * GW_LAYOUT_EDGE_TILES_BF16: the per-sample edge features of a processor stack between two blocks (bf16 mode,
 * BASELINE.json configs[2]; SURVEY.md 8(d): "halve for bf16 storage"): tiles of 64 consecutive destination-sorted edges of
 * one batch element, each tile 4 groups x 8 K-steps x 64 lanes x 8 bf16 = 32 KiB in the MFMA B-operand order
 *     byte offset ((b * ceil(E/64) + k/64) * 4 + (k%64)/16) * 8192 + s * 1024 + (16 q + k%16) * 16 + 2 i
 *     holds feature 32 s + 16 (i >> 2) + 4 q + (i & 3) of edge k of batch element b    (s < 8, q < 4, i < 8).
 * Block n writes e' in this form, block n+1 consumes it as the B operand of its layer-1 product and as its residual: half the
 * bytes of fp32 rows and every access a coalesced 1 KiB per wave instruction.  gw_edge_tiles_bytes() sizes such a buffer,
 * gw_edge_rows_to_tiles() converts rows a caller hands over. */
#define GW_LAYOUT_ROWS_F32 0
#define GW_LAYOUT_EDGE_TILES_BF16 1
/* GW_LAYOUT_ROWS_F16: layer-1 NODE PRODUCTS (X . W1_slice^T, gw_project_forward / the post products of gw_node_update_forward)
 * as fp16 rows of 256 halves (ld counts halves), values clamped to the fp16 range - bf16 mode only: the products are gathered
 * once per incident edge (~7 times on the mesh, ~77 times for a decoder source), so their bytes, not the edge features', are
 * most of what an edge update reads; fp16 keeps 11 significant bits in front of the bf16 rounding of the layer-1 activation.
 * Accepted as a projected x_src / x_dst operand by the bf16 edge update with resident weights (csrc/gw_edge16*.hip). */
#define GW_LAYOUT_ROWS_F16 2
/* GW_LAYOUT_ROWS_BF16K (v14): an AGGREGATE table (the scatter_sum of graph_net_block.py:188) as bf16 rows of 256 values in the K
 * order of the packed weight streams - position 32 s + 8 q + i of a row holds feature 32 s + 16 (i >> 2) + 4 q + (i & 3)
 * (s < 8, q < 4, i < 8; ld counts bf16 values) - i.e. exactly the 16 bytes lane q loads as its B-operand fragment of K-step s.
 * bf16 mode only: the node update rounds the aggregate to bf16 for its layer-1 product anyway (graph_net_block.py:189-190 on
 * v_mfma_f32_16x16x32_bf16), so the producer (gw_edge_update_forward with GW_EDGE_AGG_BF16K) stores what the consumer would
 * compute from fp32 rows - a quarter of the bytes written and read back (1.06 GB -> 0.27 GB per direction for the 1 degree
 * decoder at batch 16) and no conversion in the consumer.  Accepted as the raw `agg` operand of gw_node_update_forward /
 * gw_node_update_head_forward with bf16 weights. */
#define GW_LAYOUT_ROWS_BF16K 3

/* flags of gw_edge_update_forward.  GW_EDGE_DETERMINISTIC: the segment sums (scatter_sum, graph_net_block.py:188) are
 * bitwise reproducible from run to run - partial sums of segments that cross a 64-edge tile are parked in per-tile carry
 * records and added in tile order by a second small launch, instead of meeting in fp32 atomics whose order is not fixed
 * (torch_scatter's scatter_add_ on a GPU is order-nondeterministic too; this is an extra).  Needs the workspace of
 * gw_edge_update_workspace_bytes(..., flags). */
#define GW_EDGE_DETERMINISTIC 1
/* GW_EDGE_SEGMENT_TILES (v14; bf16 weights with resident kernels, every operand projected, e_res.k == 0, no e_out): `src` / `dst`
 * are a PADDED edge list of n_edges = 64 T entries in which no destination's run of edges crosses a multiple of 64 ("segment-
 * aligned tiles": assimilator_decoder.py:92-103 gives every grid node 7 or 6 consecutive edges, so 9 nodes = 63 columns fill a
 * tile).  dst[k] < 0 marks a padding column (src[k] must still be a valid row; rows of batch-shared per-edge tables are indexed by
 * the padded position k; edge tiles cover the padded list).  Every destination segment is then complete inside one tile:
 *   - e_res.k == 0 (no residual, no e_out; decoder): agg rows of destinations that have edges are WRITTEN (=, plain stores - no
 *     atomics, bitwise reproducible), rows of destinations without edges are not touched;
 *   - e_in = per-sample bf16 edge tiles (raw) with e_res = the same tiles (a processor block, graph_net_block.py:293-301): agg rows
 *     are UPDATED in place, agg[dst] += sum of LayerNorm(.) over the destination's edges WITHOUT the residual - the caller hands
 *     over the previous block's aggregate, whose rows are the segment sums of this block's residual (e of block n = e' of block
 *     n - 1), so the buffer always holds sum(e') (plain load / add / store; at most 16 destinations per tile);
 *   - every operand projected with a batch-shared residual (first processor block): as without the flag (agg += by atomics on a
 *     zero fill), the padding columns are skipped.
 * GW_EDGE_AGG_BF16K (with GW_EDGE_SEGMENT_TILES, no residual): `agg` points to bf16 rows in K order (GW_LAYOUT_ROWS_BF16K).
 * GW_EDGE_SEGMENT_SPLIT (with GW_EDGE_SEGMENT_TILES, no residual, fp32 agg): a destination with more than 64 edges (a polar
 * mesh cell of the encoder graph, encoder.py:75-104) is allowed: its run starts a fresh tile and continues over whole tiles; the
 * pieces are partial sums that are ADDED with fp32 atomics, all other rows are written - agg must be zero-filled by the caller. */
#define GW_EDGE_SEGMENT_TILES 2
#define GW_EDGE_AGG_BF16K 4
#define GW_EDGE_SEGMENT_SPLIT 8

/* Library / ABI version and last error text (thread local). */
int gw_version(void);
const char* gw_last_error(void);
/* Debug/profiling aid (no reference counterpart): while `buffer` != NULL, launches of family `kind` (0 mlp, 1 edge
 * update, 2 node update, 3 project) write 16 x uint64 per workgroup: s_memtime stamps of the kernel phases [0..6],
 * HW_ID [8], XCC_ID [9], block index [10].  buffer: device memory, capacity_workgroups * 16 * 8 bytes. */
int gw_debug_timestamps(void* buffer, int capacity_workgroups, int kind);

/* ---- weight packing ------------------------------------------------------------------------------------
 * Packed size in floats of the [k_lo, k_hi) column slice of an nn.Linear weight with `n_out` rows, padded to
 * 16-row tiles / 16-column groups (graph_net_block.py:45-49 creates the Linear layers being packed). */
size_t gw_packed_floats(int n_out, int k_lo, int k_hi);
/* w: device pointer to [n_out, k_total] fp32 (nn.Linear.weight); out: gw_packed_floats() floats. */
int gw_pack_linear(const float* w, int n_out, int k_total, int k_lo, int k_hi, float* out, void* stream);
/* bf16 form of the packed stream (byte size / packing); same arguments, out receives gw_packed_bytes_bf16() bytes. */
size_t gw_packed_bytes_bf16(int n_out, int k_lo, int k_hi);
int gw_pack_linear_bf16(const float* w, int n_out, int k_total, int k_lo, int k_hi, void* out, void* stream);
/* (v16) split form (GW_DTYPE_BF16X3): per 32-wide K-step the bf16 hi fragments of all row tiles, then their lo fragments;
 * out receives gw_packed_bytes_bf16x3() bytes (twice the bf16 stream). */
size_t gw_packed_bytes_bf16x3(int n_out, int k_lo, int k_hi);
int gw_pack_linear_bf16x3(const float* w, int n_out, int k_total, int k_lo, int k_hi, void* out, void* stream);
/* Zero-pad a vector (bias / LayerNorm gamma, beta) to a multiple of 32 floats. out has gw_padded_n(n). */
int gw_padded_n(int n);
int gw_pad_vector(const float* v, int n, float* out, void* stream);
/* (v13) Every matrix slice and vector of one MLP (or any other set) packed by ONE launch: what MLP.__init__ creates
 * (graph_net_block.py:45-61) is 3-5 Linear layers and a LayerNorm, i.e. ~10 gw_pack_linear / gw_pad_vector launches of a few
 * microseconds each per MLP and weight version - 27 MLPs per forecaster, every training step.  A matrix item is addressed by
 * strides, element (f, k) of the slice = w[f * stride_f + k * stride_k], so a column slice of nn.Linear.weight is
 * {w + k_lo, k_total, 1} and the transposed block the backward's input-gradient products stream ("Linear" that maps
 * gradients back, W[:, lo:hi]^T) is {w + lo, 1, k_total} - no transposed copy is materialised.  Rows n_out.. of the last
 * 16-row tile quad and input features kseg.. of the last K-step are zero.  The item arrays are HOST memory (copied into the
 * launch); at most GW_PACK_MAX_ITEMS matrices and GW_PACK_MAX_ITEMS vectors per call. */
#define GW_PACK_MAX_ITEMS 16
typedef struct gw_pack_item {
  const float* w;      /* device pointer to element (0, 0) of the slice */
  int64_t stride_f;    /* floats between consecutive output features (rows of nn.Linear.weight: k_total) */
  int64_t stride_k;    /* floats between consecutive input features (1) */
  int32_t n_out;       /* output features of the slice */
  int32_t kseg;        /* input features of the slice */
  int32_t rows;        /* rows of the packed stream, >= n_out (0 = n_out): an output head with n_out < 80 features is packed as
                          80 rows, the tile count its kernel variant walks; rows n_out.. are zero */
  int32_t reserved;
  void* out;           /* gw_packed_floats(rows, 0, kseg) floats, or gw_packed_bytes_bf16 / _bf16x3(rows, 0, kseg) bytes */
} gw_pack_item;
typedef struct gw_pad_item {
  const float* v;      /* device pointer, n floats */
  int32_t n;
  int32_t n_out;       /* entries written, >= n (0 = n), rounded up to gw_padded_n(); entries n.. are zero */
  float* out;          /* gw_padded_n(max(n, n_out)) floats */
} gw_pad_item;
int gw_pack_many(int32_t weight_dtype, int32_t n_mats, const gw_pack_item* mats, int32_t n_vecs, const gw_pad_item* vecs,
                 void* stream);

/* One input operand of a fused MLP ("segment" of the concatenated input). */
typedef struct gw_operand {
  const float* ptr;     /* table base                                                          */
  const int32_t* index; /* per-column row index within a batch element, NULL = identity         */
  int32_t rows_per_batch; /* rows of the table per batch element, 0 = table shared by the batch */
  int32_t ld;           /* row stride in floats                                                 */
  int32_t k;            /* valid input features taken from each row (0 = operand is all zeros:  */
                        /* its weight slice is skipped, exact since 0*W == 0)                    */
  int32_t projected;    /* 1 = rows already hold X . W1_slice^T (from gw_project_forward): they */
                        /* are gather-added into the layer-1 accumulator, no MFMA pass           */
  int32_t layout;       /* GW_LAYOUT_*: ROWS_F32 everywhere except the e_in / e_res operands of  */
                        /* gw_edge_update_forward, which may be EDGE_TILES_BF16 (ptr = tile      */
                        /* buffer; rows_per_batch = n_edges: one tile set per batch element, 0:  */
                        /* one set shared by the batch; ld / index unused, k = 256)              */
} gw_operand;

/* A 3+ layer MLP in packed form: Linear(k_in,h) ReLU [Linear(h,h) ReLU]*n_mid Linear(h,n_out) [LayerNorm]. */
typedef struct gw_mlp_weights {
  const float* w1[3];  /* packed slices of layer-1 weight, one per operand (NULL if operand k == 0) */
  const float* b1;     /* padded bias [h]                                                           */
  const float* w_mid;  /* n_mid packed [h,h] matrices, contiguous                                   */
  const float* b_mid;  /* n_mid padded biases                                                       */
  const float* w_out;  /* packed [n_out, h]                                                         */
  const float* b_out;  /* padded bias                                                               */
  const float* ln_gamma; /* padded, NULL = no LayerNorm (eps = 1e-5, biased variance)               */
  const float* ln_beta;
  int32_t hidden;      /* 128 or 256 */
  int32_t n_mid;       /* hidden_layers - 1 */
  int32_t n_out;       /* 256, or <= 80 for the decoder head */
  int32_t weight_dtype; /* GW_DTYPE_F32: streams from gw_pack_linear; GW_DTYPE_BF16: gw_pack_linear_bf16; GW_DTYPE_BF16X3: gw_pack_linear_bf16x3 */
  int32_t ln_width;    /* features LayerNorm normalises over; 0 = n_out.  Narrower models (node/edge width < 256,
                          graph_net_block.py:234-244 defaults to 128) run zero-padded to 256: their statistics then span
                          the first ln_width features only (fp32 weights) */
  int32_t k_in;        /* (v15) input features the layer-1 slices were packed for, summed over the operands; 0 = not recorded (MANDATORY - as is
                          out_rows - for the `head` argument of gw_node_update_head_forward, which rejects a zeroed struct).
                          Entry points that stream a FIXED number of K-steps from w1 (gw_node_update_head_forward: the
                          head's 256 inputs) refuse anything else instead of reading past the packed buffer */
  int32_t out_rows;    /* (v15) rows w_out / b_out were packed with (gw_pack_linear rows > n_out: zero rows of an output
                          head); 0 = gw_padded_n(n_out).  gw_node_update_head_forward requires 80 */
} gw_mlp_weights;

struct gw_activation_save; /* training only, defined with the backward entry points below; NULL in inference */

/* ---- MLP.forward (graph_net_block.py:63-77) applied to rows --------------------------------------------
 * y[c, :] = MLP(x[c, :k]) (+ residual[c, :n_out]);   c in [0, n_rows).
 * Used for Encoder.node_encoder (encoder.py:205), the three edge encoders (encoder.py:206-208,235-241,
 * assimilator_decoder.py:175-177) and AssimilatorDecoder.node_decoder + the Decoder residual
 * (assimilator_decoder.py:197, decoder.py:93).  Supported k: <= 16, <= 112, or exactly 256. */
int gw_mlp_forward(int64_t n_rows, int32_t rows_per_batch, const gw_operand* x, const gw_mlp_weights* w,
                   const gw_operand* residual /* may be NULL */, float* out, int32_t out_ld,
                   const struct gw_activation_save* save /* may be NULL */, void* stream);

/* The same MLP whose output rows y are, while still in registers, multiplied by n_post (1..4) packed [256, 256] slices:
 * post_out[s][c] = y[c] . post_w[s]^T (rows of 256; post_layout GW_LAYOUT_ROWS_F32 / _F16) - Encoder.node_encoder on the grid
 * rows (encoder.py:205) followed by the x[row] slice of the encoder block's edge MLP layer 1 (graph_net_block.py:131-134: one
 * edge per grid node, so the product costs what the raw operand would cost inside the edge kernel).  out may be NULL when only
 * the products are wanted (the encoder drops the grid rows, encoder.py:219-223).  bf16 / bf16x3 weights, hidden 256, 256 outputs with
 * LayerNorm, 33..128 input features. */
int gw_mlp_post_forward(int64_t n_rows, int32_t rows_per_batch, const gw_operand* x, const gw_mlp_weights* w,
                        float* out /* may be NULL */, int32_t out_ld, int32_t n_post, const float* const* post_w,
                        void* const* post_out, int32_t post_layout, void* stream);

/* (v13) Backward of the Linear / ReLU chain of an MLP (graph_net_block.py:45-61; what autograd runs for loss.backward(),
 * train/run.py:517-519, as one addmm-backward + threshold_backward pair per layer) in one launch, register-resident like the
 * forward: d_0 = d [n_rows, 256 (ld d_ld)];  d_{i+1} = (d_i . W_i) * (mask_i > 0) for i < n_chain (<= 2), each stored to
 * chain_out[i] [n_rows, 256] (the weight-gradient products read them); then fan_out[s] = d_{n_chain} . Wf_s for s < n_fan (<= 3):
 * the input gradients of the first Linear's operand blocks.  chain_w / fan_w: packed TRANSPOSED 256 x 256 blocks
 * (gw_pack_many with {w + lo, 1, k_total}); chain_mask[i]: the ReLU output that fed layer i [n_rows, 256] (gw_activation_save).
 * fp32 streams. */
int gw_mlp_chain_backward(int64_t n_rows, const float* d, int32_t d_ld, int32_t n_chain, const float* const* chain_w,
                          const float* const* chain_mask, float* const* chain_out, int32_t n_fan, const float* const* fan_w,
                          float* const* fan_out, void* stream);
/* (v18) The same chain on split operands (mixed-precision training, GW_DTYPE_BF16X3): chain_w / fan_w are the packed transposed
 * blocks in the split stream (gw_pack_many with GW_DTYPE_BF16X3); every product is the forward's three bf16 MFMAs on (hi, lo)
 * pairs, the gradient rows stay in registers between the products.  d, masks and outputs are fp32 rows as above. */
int gw_mlp_chain_backward_bf16x3(int64_t n_rows, const float* d, int32_t d_ld, int32_t n_chain, const void* const* chain_w,
                                 const float* const* chain_mask, float* const* chain_out, int32_t n_fan, const void* const* fan_w,
                                 float* const* fan_out, void* stream);

/* (v19) native_layer_norm_backward + that chain in one launch (what autograd runs behind MLP.forward's LayerNorm,
 * graph_net_block.py:59-61, under loss.backward()): dn [n_rows, 256 (ld dn_ld)] is the gradient at the OUTPUT of the LayerNorm
 * (width 256, eps 1e-5, biased variance), y the saved pre-norm rows [n_rows, 256]; dy [n_rows, 256] receives the gradient at the
 * norm's input (the last Linear's weight-gradient product reads it) and is the chain's d_0 without being read back;
 * dgamma / dbeta [256] are accumulated (+=).  y == NULL: no LayerNorm, dn is d_0 (gamma, dgamma, dbeta, dy unused).
 * With the LayerNorm the input gradient may be GATHERED by the launch (the index_select backward of scatter_sum,
 * graph_net_block.py:188: every edge row receives its destination's row of the aggregate's gradient): dn_idx [dn_idx_n] (NULL:
 * row c reads row c of dn) - row c = b * dn_idx_n + k reads dn[b * dn_table_rows_pb + dn_idx[k]] - plus row c of dn_add
 * [n_rows, 256 (ld dn_add_ld)] (may be NULL: the gradient of e' where the block exposes it); the [n_rows, 256] table of gathered
 * rows is then never written.
 * The chain arguments are those of gw_mlp_chain_backward_bf16x3, plus three things autograd does with separate kernels:
 * dz_colsum [256] (may be NULL) += column sums of the last chain gradient - the first Linear's bias gradient
 * (addmm backward's sum over rows); fan_add[s] (array or entries may be NULL; rows [n_rows, 256 (ld fan_add_ld)]) is added
 * to fan_out[s] before it is stored - the gradient of a tensor that is both an operand of the first Linear and the block's
 * residual (EdgeProcessor: graph_net_block.py:131-137) arrives as one row; bit s of fan_add_dn_mask: that joining gradient is
 * the launch's own input gradient row (dn as gathered).
 * weight_dtype: GW_DTYPE_F32 or GW_DTYPE_BF16X3 - the dtype of the packed streams. */
int gw_mlp_ln_chain_backward(int32_t weight_dtype, int64_t n_rows, const float* dn, int32_t dn_ld, const int32_t* dn_idx,
                             int32_t dn_idx_n, int32_t dn_table_rows_pb, const float* dn_add, int32_t dn_add_ld, const float* y,
                             const float* gamma, float* dgamma, float* dbeta, float* dy, int32_t n_chain, const void* const* chain_w,
                             const float* const* chain_mask, float* const* chain_out, float* dz_colsum, int32_t n_fan,
                             const void* const* fan_w, float* const* fan_out, const float* const* fan_add, int32_t fan_add_ld,
                             uint32_t fan_add_dn_mask, void* stream);

/* ---- layer-1 split: cat[x_s, x_d, e] . W1^T == x_s . Ws^T + x_d . Wd^T + e . We^T ------------------------
 * (graph_net_block.py:131-134 concatenates and multiplies; the products over node tables are shared by the ~7
 * edges incident to a node, and the ones over batch-independent tables are cacheable.)
 * out_s[c, :] = x[c, :256] . W_s^T for s < n_slices (<= 4); W_s = packed [256, 256] slices from gw_pack_linear. */
int gw_project_forward(int64_t n_rows, int32_t rows_per_batch, const gw_operand* x, int32_t n_slices,
                       const float* const* w_slices, void* const* outs, int32_t out_ld,
                       int32_t out_layout /* GW_LAYOUT_ROWS_F32, or GW_LAYOUT_ROWS_F16 (bf16 slices; out_ld in halves) */,
                       int32_t weight_dtype /* GW_DTYPE_* of the slices */,
                       const float* relu_mask /* NULL, or [n_rows, 256]: out *= (relu_mask > 0) - ReLU backward fused into an
                                                  input-gradient product (backward pass; single fp32 slice) */,
                       float* zero_rows /* NULL, or [n_rows, 256] filled with zeros on the side: the aggregate buffer of the
                                           edge update that consumes these products (saves a fill launch; fp32) */,
                       void* stream);

/* ---- EdgeProcessor.forward + scatter_sum (graph_net_block.py:131-137 and :188) --------------------------
 * For every batch element b and edge e (dst-sorted):
 *   e_new = LN(MLP(cat[x_src[b, src[e]], x_dst[b, dst[e]], e_in[b, e]])) + e_res[b, e]
 *   agg[b, dst[e], :] += e_new                         (agg must be zero-filled by the caller)
 * and, if e_out != NULL, e_out[b, e, :] = e_new.  Feature width is 256.  Each of x_src / x_dst / e_in may be
 * raw rows, pre-projected rows (operand.projected) or zeros (k == 0); e_res is the raw edge feature row (the residual of
 * graph_net_block.py:135) - or k == 0 for "none": a caller that wants only the aggregate of batch-shared edge features (the
 * decoder, assimilator_decoder.py:195 drops e') may add their per-destination sums into agg beforehand instead,
 * sum(LN(.) + e) = sum(LN(.)) + sum(e)  (bf16 weights with resident kernels in atomics mode, or bf16x3 weights, or float32
 * weights with nothing raw, one or two projected fp32-row operands, one middle layer, LayerNorm over 256 features, atomics mode - the
 * decoder-form kernel of csrc/gw_edge_stream.hip; e_out == NULL, no save). */
int gw_edge_update_forward(int32_t batch, int32_t n_edges, const int32_t* src, const int32_t* dst,
                           const gw_operand* x_src, const gw_operand* x_dst, const gw_operand* e_in,
                           const gw_operand* e_res, const gw_mlp_weights* w,
                           void* e_out /* NULL, or fp32 rows [batch*n_edges,256], or bf16 edge tiles (e_out_layout) */,
                           int32_t e_out_layout /* GW_LAYOUT_* of e_out */, float* agg /* [batch*n_dst,256] (GW_EDGE_AGG_BF16K: bf16) */,
                           int32_t n_dst, const struct gw_activation_save* save /* may be NULL */,
                           void* workspace /* may be NULL */, size_t workspace_bytes, int32_t flags /* GW_EDGE_* */, void* stream);
/* Edge tiles (GW_LAYOUT_EDGE_TILES_BF16) are consumed and produced by the bf16 path with register-resident weights only:
 * bf16 weights, one middle layer, x_src / x_dst pre-projected or zero, and the workspace of gw_edge_update_workspace_bytes. */
size_t gw_edge_tiles_bytes(int32_t batch, int32_t n_edges);
/* rows [batch (rows_per_batch > 0) or shared (0)][n_edges, ld] fp32 -> tiles (bf16, round to nearest even; padding edges 0). */
int gw_edge_rows_to_tiles(int32_t batch, int32_t n_edges, const float* rows, int32_t rows_per_batch, int32_t ld, void* tiles,
                          void* stream);
/* Scratch device memory (16-byte aligned, contents irrelevant) gw_edge_update_forward needs for these operands and flags:
 * the bf16 path with a raw edge operand (bf16 tiles) stages the layer-1 activations of all tiles between its two launches
 * (32 KiB per 64 edges and batch element); deterministic segment sums park one carry record per tile.  0 = none needed
 * (e.g. the bf16 path whose operands are all projected gathers them inside its one persistent launch); the library never
 * allocates (the caller's allocator owns all device memory). */
size_t gw_edge_update_workspace_bytes(int32_t batch, int32_t n_edges, const gw_operand* x_src, const gw_operand* x_dst,
                                      const gw_operand* e_in, const gw_mlp_weights* w, int32_t flags);

/* ---- The fp32 encoder stage in one launch (csrc/gw_encoder_fused.hip; added without a version bump) ------------------
 *   xg[b, src[k]] = node_encoder(features[b, src[k]])                  (encoder.py:199-205, never written)
 *   agg[b, dst[k]] += LN(MLP_e(cat[xg[b, src[k]], x_dst[b, dst[k]], e_in[k]])) [+ e_res[k]]
 * for graphs with one edge per source row in real use (the result does not depend on it: a source row that occurs twice is
 * encoded twice).  features: raw fp32 rows of 17..112 floats (index NULL, rows_per_batch = grid rows per batch element);
 * w_node: float32, one middle layer, widths 256, LayerNorm over 256; w_edge as in gw_edge_update_forward with its x_src slice
 * w1[0] packed, x_dst / e_in projected fp32 rows (one of them may have k == 0); e_res: 256-wide fp32 rows, or k == 0 (no
 * residual: the caller adds the segment sums of its batch-shared e).  save must be NULL and flags 0 (atomics mode on row
 * tiles); every other combination returns GW_E_UNSUPPORTED.  With e_res the aggregate is bit for bit the one of
 * gw_mlp_forward followed by gw_edge_update_forward.  agg must be zeroed. */
int gw_encoder_fused_forward(int32_t batch, int32_t n_edges, const int32_t* src, const int32_t* dst, const gw_operand* features,
                             const gw_mlp_weights* w_node, const gw_operand* x_dst, const gw_operand* e_in, const gw_operand* e_res,
                             const gw_mlp_weights* w_edge, float* agg /* [batch*n_dst,256] */, int32_t n_dst,
                             const struct gw_activation_save* save /* must be NULL */, int32_t flags /* must be 0 */, void* stream);

/* ---- NodeProcessor.forward after aggregation (graph_net_block.py:189-191) -------------------------------
 *   x_new[b, j] = LN(MLP(cat[x[b, j], agg[b, j]])) + x_res[b, j]
 * x may be raw, pre-projected or zeros (k == 0: the decoder's lat/lon rows are zeros, assimilator_decoder.py:84,
 * 190 - the x-slice of layer 1 is skipped); x_res = raw node rows for the residual (NULL or k == 0: none).  With bf16
 * weights a pre-projected x may be fp16 product rows (GW_LAYOUT_ROWS_F16, ld in halves); every other operand of the row-wise
 * entry points is fp32 rows - any other layout is rejected; agg may also be bf16 rows in K order (GW_LAYOUT_ROWS_BF16K, bf16
 * weights, ld in bf16 values, no index). */
int gw_node_update_forward(int64_t n_rows, int32_t rows_per_batch, const gw_operand* x, const gw_operand* x_res,
                           const gw_operand* agg, const gw_mlp_weights* w, float* x_out, int32_t out_ld,
                           const struct gw_activation_save* save /* may be NULL */,
                           int32_t n_post /* 0..4 */, const float* const* post_w, void* const* post_out,
                           int32_t post_layout /* GW_LAYOUT_ROWS_F32, or GW_LAYOUT_ROWS_F16 (bf16 weights) */,
                           float* zero_rows /* may be NULL */, void* stream);
/* n_post > 0: while the new rows are still in registers they are multiplied by n_post packed [256, 256] slices (packing and
 * dtype of w) and the products written to post_out[s] [n_rows, 256]: post_out[s][j] = x_new[j] . post_w[s]^T - the layer-1
 * products of the NEXT block's edge MLP over the node table (see gw_project_forward), so that GraphProcessor's loop
 * (graph_net_block.py:293-301) needs no projection launch between blocks.  zero_rows: [n_rows, 256] filled with zeros on the
 * side (the next block's aggregate buffer).  Inference only (save must be NULL), out_ld 256. */

/* (v17) Which kernel form gw_node_update_forward gives a launch of n_rows rows with fp32 / bf16x3 weights (fp32 row tables,
 * one middle layer, LayerNorm over 256 features or none, no activation saves): 1, 2 or 3 = the row-split kernels of
 * csrc/gw_noders.hip with that many 16-column groups per workgroup (mesh-sized launches: at most one round of 48-column
 * workgroups on the 256 CUs), 0 = the 64-column kernels.  Pure host logic (no GPU needed): graph_weather_amd/routes.py keeps the
 * same table and tests/test_routes.py compares the two. */
int gw_node_update_row_split_groups(int64_t n_rows);

/* ---- NodeProcessor.forward followed by the output head, one launch (fp32 since v17; bf16; bf16x3) ---------------------
 * AssimilatorDecoder.forward after its edge update (assimilator_decoder.py:195-200) + the Decoder residual (decoder.py:93):
 *   x_new[j] = LN(MLP_node(cat[x[j], agg[j]]))            (graph_net_block.py:189-191; the decoder's rows are zeros: no x_res)
 *   out[j, :n] = MLP_head(x_new[j]) + residual[j, :n]     (node_decoder 256 -> 128 -> 128 -> n <= 80 features, no norm)
 * x_new stays in registers: the [rows, 256] table between the two MLPs is neither written nor read.
 * Packed sizes the kernel streams unconditionally - checked through head->k_in == 256 and head->out_rows == 80 (v15):
 * head->w1[0] = [128, 256] slice (8 K-steps x 8 row tiles), head->w_mid = [128, 128], head->w_out / b_out packed with rows = 80.
 * Both MLPs in the same weight dtype.  fp32: the same arithmetic in the same order as gw_node_update_forward followed by
 * gw_mlp_forward with a residual - bitwise their result (tests/test_gpu_round6.py). */
int gw_node_update_head_forward(int64_t n_rows, int32_t rows_per_batch, const gw_operand* x, const gw_operand* agg,
                                const gw_mlp_weights* w, const gw_mlp_weights* head, const gw_operand* residual /* may be NULL */,
                                float* out, int32_t out_ld, void* stream);

/* ---- NormalizedMSELoss.forward (losses.py:66-94, normalize on/off) ---------------------------------------
 * loss = mean_{b,n}( w_lat[n / num_lon] * mean_c( (pred-target)^2 [/ var_c] ) ); *loss_out must be zeroed. */
int gw_normalized_mse_forward(const float* pred, const float* target,
                              const float* inv_var /* NULL, [c] (inv_var_full 0) or [batch, nodes, c] (inv_var_full 1) */,
                              int32_t inv_var_full, const float* lat_weights, int32_t num_unique_lat, int32_t batch, int32_t nodes,
                              int32_t channels, float* loss_out, void* stream);

/* =====================================================================================================================
 * Backward / training step (reference: autograd through the same modules + torch.optim.AdamW, train/run.py:509-521;
 * SURVEY.md 8f row 1).  The forward entry points above take an optional gw_activation_save: when given, the fused
 * kernels also write the activations autograd would have saved; the backward is then composed from the generic
 * kernels below (all fp32, matrix products on the fp32 MFMA like the forward).
 * ===================================================================================================================== */

/* Activations written by a forward call for its backward (all row-major fp32, one row per column of the launch):
 * hidden[l] = relu output of Linear l (l = 0 .. n_mid), hidden_ld floats per row (>= hidden width);
 * pre_norm = output of the last Linear before LayerNorm (NULL when the MLP has no norm). */
typedef struct gw_activation_save {
  float* hidden;        /* [(n_mid + 1), n_rows, hidden_ld] */
  int64_t hidden_stride; /* floats between consecutive hidden layers */
  int32_t hidden_ld;
  float* pre_norm;      /* [n_rows, 256] ([n_rows, 80] for an output head with n_out <= 80, zero padded) or NULL */
} gw_activation_save;

#define GW_GEMM_NN 0 /* C[m][n]  = sum_k A[m][k] * B[k][n]   (input gradients:  dX = dZ . W)                         */
#define GW_GEMM_TN 1 /* C[m][n] += sum_k A[k][m] * B[k][n]   (weight gradients: dW += dZ^T . X; C must hold the sum) */
#define GW_GEMM_TN_BF16X3 2 /* (v16) GW_GEMM_TN with split-operand products (both operands as bf16 hi / lo pairs, three bf16 MFMAs per
                               product, fp32 accumulate: the weight-gradient GEMMs of the mixed-precision training step); any
                               shape, leading dimension and alignment (v19; before: multiples of 128 only, other shapes on
                               the fp32 kernel) */
int gw_gemm_f32(int32_t mode, int64_t m, int32_t n, int64_t k, const float* a, int32_t lda, const float* b, int32_t ldb,
                float* c, int32_t ldc, float* colsum_a /* TN only, may be NULL: colsum_a[m] += sum_k A[k][m] (bias gradient; n == 0 too) */,
                void* stream);
/* nn.ReLU backward fused with the nn.Linear bias gradient: dz = dh * (h > 0) (h NULL: dz = dh), db[c] += sum_r dz[r][c].
 * dz may alias dh or be NULL (bias gradient only); db may be NULL.  Any width (above 256: wide models, csrc/gw_wide.hip). */
int gw_relu_backward(int64_t rows, int32_t width, const float* dh, int32_t ld_dh, const float* h, int32_t ld_h, float* dz,
                     int32_t ld_dz, float* db, void* stream);
/* nn.LayerNorm(width, eps 1e-5) backward from the saved pre-norm rows y: dy; dgamma += , dbeta += (may be NULL).
 * width 256: the message-passing MLPs; other widths <= 256: LayerNorm on an output head (regional_forecast.py:223-230);
 * 257..4096: wide models. */
int gw_layernorm_backward(int64_t rows, int32_t width, const float* dn, int32_t ld_dn, const float* y, int32_t ld_y,
                          const float* gamma, float* dy, int32_t ld_dy, float* dgamma, float* dbeta, void* stream);
/* Dual of the segment sum (graph_net_block.py:188): out[b, k, :] = table[b, idx[k], :] (+ add[b, k, :]); 256-float rows;
 * idx NULL = identity; rows_per_batch 0 = table shared by the batch. */
int gw_gather_rows(int32_t batch, int32_t n_idx, const float* table, int32_t rows_per_batch, const int32_t* idx,
                   const float* add, float* out, void* stream);
/* Dual of the x[row] / x[col] gathers (MetaLayer, graph_net_block.py:221-228):
 * out[bo, n, :] (+)= sum_{b} sum_{i in [ptr[n], ptr[n+1])} rows[b, perm[i], :]; perm NULL = identity;
 * batch_out == batch: per sample; batch_out == 1: summed over the batch too (gradient of a batch-shared table). */
int gw_segment_sum_rows(int32_t batch, int32_t batch_out, int32_t n_seg, const float* rows, int32_t rows_per_batch_in,
                        const int32_t* perm, const int32_t* ptr, float* out, int32_t accumulate, void* stream);
/* NormalizedMSELoss backward (losses.py:66-94): dpred = dloss * d loss / d pred; refuses the shapes the forward refuses. */
int gw_normalized_mse_backward(const float* pred, const float* target, const float* inv_var, int32_t inv_var_full,
                               const float* lat_weights,
                               int32_t num_unique_lat, int32_t batch, int32_t nodes, int32_t channels, const float* dloss,
                               float* dpred, void* stream);
/* torch.optim.AdamW step (decoupled weight decay, bias correction with `step` >= 1) on a flat fp32 buffer. */
int gw_adamw_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int32_t step, void* stream);

/* BoundaryNudgingLayer (regional_forecast.py:44-132) on rows of in = [regional (feat) | global context (feat) | prior (1)]:
 * alpha = clamp(prior + w2 . relu(W1 . in + b1) + b2, 0, 1); out = (1 - alpha) regional + alpha context.
 * w1t = W1^T ([2 feat + 1, hidden] row-major), w2 [hidden], b2 [1]; feat, hidden <= 256. */
int gw_nudging_forward(int64_t rows, int32_t feat, int32_t hidden, const float* in, int32_t ld_in, const float* w1t, const float* b1,
                       const float* w2, const float* b2, float* out, void* stream);
/* Its backward for dout [rows, feat]: d_in[:, 0:feat] = gradient of the regional columns (other columns untouched),
 * dz [rows, hidden] = gradient at the hidden pre-activations, hid [rows, hidden] = relu(hidden), dcorr [rows] = gradient at the
 * MLP output; the parameter gradients are then dW1 += dz^T in, db1 += colsum dz, dw2 += dcorr^T hid, db2 += sum dcorr
 * (gw_gemm_f32 TN).  w1 = W1 ([hidden, 2 feat + 1] row-major). */
int gw_nudging_backward(int64_t rows, int32_t feat, int32_t hidden, const float* in, int32_t ld_in, const float* w1, const float* w1t,
                        const float* b1, const float* w2, const float* b2, const float* dout, float* d_in, int32_t ld_din, float* dz,
                        float* hid, float* dcorr, void* stream);

/* =====================================================================================================================
 * Models wider than 256 features (the reference's training script builds 1024-wide ones, train/run.py:493-497) run layer
 * by layer on the generic kernels below (csrc/gw_wide.hip) instead of the fused ones: same arithmetic as graph_net_block.py,
 * nothing fused across layers.  All fp32 row-major, any width.
 * ===================================================================================================================== */
/* nn.Linear (+ nn.ReLU): out[r, :n] = act(x[r, :k] . w^T + bias); w = nn.Linear.weight as it lies in memory ([n, k], row
 * stride ldw); bias may be NULL; relu 0 / 1.  fp32 MFMA, fp32 accumulate. */
int gw_linear_forward(int64_t rows, int32_t k, int32_t n, const float* x, int32_t ldx, const float* w, int32_t ldw, const float* bias,
                      int32_t relu, float* out, int32_t ldo, void* stream);
/* The same Linear with up to three row tables added before the activation:
 *   out[m] = act(x[m] . w^T + bias + sum_i table_i[b * rows_pb_i + idx_i[k]]),  (b, k) = (m / rows_per_batch, m % rows_per_batch)
 * (idx_i NULL: k itself; rows_pb_i 0: table shared by the batch).  This is the layer-1 split of the fused kernels for wide
 * models - cat[x_s, x_d, e] . W1^T = (x_s . Ws^T)[src] + (x_d . Wd^T)[dst] + e . We^T: node products are made once per node and
 * gathered per edge in the epilogue of the edge-level product.  k == 0 (x, w NULL): no product, only bias + gathered rows. */
int gw_linear_gather_forward(int64_t rows, int32_t rows_per_batch, int32_t k, int32_t n, const float* x, int32_t ldx, const float* w,
                             int32_t ldw, const float* bias, int32_t n_add, const float* const* add_table, const int32_t* const* add_idx,
                             const int32_t* add_ld, const int32_t* add_rows_pb, int32_t relu, float* out, int32_t ldo, void* stream);
/* nn.LayerNorm(width, eps 1e-5, affine) (+ res, the residual add of graph_net_block.py:135/:191; res_period > 0: residual rows
 * shared by the batch, row m reads res[m % res_period]); width <= 4096. */
int gw_layernorm_forward(int64_t rows, int32_t width, const float* y, int32_t ld_y, const float* gamma, const float* beta,
                         const float* res, int32_t ld_res, int64_t res_period, float* out, int32_t ld_out, void* stream);
/* out = a + b (residual add behind an MLP without norm). */
int gw_add_rows(int64_t rows, int32_t width, const float* a, int32_t lda, const float* b, int32_t ldb, float* out, int32_t ldo,
                void* stream);
/* gw_gather_rows / gw_segment_sum_rows for rows of any width (row strides ld / ldo); the segment sum walks the CSR in one
 * fixed order (no atomics: bitwise reproducible). */
int gw_gather_rows_wide(int32_t batch, int32_t n_idx, int32_t width, const float* table, int32_t ld, int32_t rows_per_batch,
                        const int32_t* idx, float* out, int32_t ldo, void* stream);
int gw_segment_sum_rows_wide(int32_t batch, int32_t batch_out, int32_t n_seg, int32_t width, const float* rows, int32_t ld,
                             int32_t rows_per_batch_in, const int32_t* perm, const int32_t* ptr, float* out, int32_t ldo, void* stream);
/* The two calls above for copies that come in groups (B samples x N members, copy c = b N + n): every table has a share count
 * s_i >= 1 and copy c reads block c / s_i (s_i 1: one block per copy; s_i = N: one block per sample; rows_pb_i 0: one block for
 * all) - gw_linear_gather_forward is the case of every s_i = 1.  gw_segment_sum_rows_grouped is the gradient of such a table:
 * out [batch / share, n_seg, width], block g the sum of copies g share .. g share + share - 1 in copy order, each walked in CSR
 * order (batch a multiple of share); gw_segment_sum_rows_wide is share = 1 (batch_out = batch) and share = batch (batch_out = 1),
 * with the same bits. */
int gw_linear_gather_grouped_forward(int64_t rows, int32_t rows_per_batch, int32_t k, int32_t n, const float* x, int32_t ldx, const float* w,
                                     int32_t ldw, const float* bias, int32_t n_add, const float* const* add_table,
                                     const int32_t* const* add_idx, const int32_t* add_ld, const int32_t* add_rows_pb,
                                     const int32_t* add_share, int32_t relu, float* out, int32_t ldo, void* stream);
int gw_segment_sum_rows_grouped(int32_t batch, int32_t share, int32_t n_seg, int32_t width, const float* rows, int32_t ld,
                                int32_t rows_per_batch_in, const int32_t* perm, const int32_t* ptr, float* out, int32_t ldo, void* stream);

/* =====================================================================================================================
 * PhysicalConstraintLayer (graph_weather/models/layers/constraint_layer.py) behind the decoder (forecast.py:234-246),
 * csrc/gw_constraint.hip.  The reference's grid round trip (graph_to_grid / grid_to_graph, last writer wins) reduces to a
 * gather through a node -> row map: node n reads row map[n] of hr (the decoder output as grid rows) and of lr (the input's
 * first channels).  With h = hr[b, map[n], c], l = lr[b, map[n], c] and means over all `nodes` nodes:
 *   GW_CONSTRAINT_ADDITIVE        out[b, n, c] = h + (l - mean_m hr[b, map[m], c])
 *   GW_CONSTRAINT_MULTIPLICATIVE  out[b, n, c] = h * (mean_m lr[b, map[m], c] / (mean_m hr[b, map[m], c] + 1e-8))
 *   GW_CONSTRAINT_SOFTMAX, f = 1  out[b, n, c] = e * (l * (1 / e)), e = exp(exp_factor * h)   (the reference's order of
 *                                 operations: inf / NaN exactly where it overflows)
 *   GW_CONSTRAINT_SOFTMAX, f > 1  E = exp(exp_factor * hr) on the grid_h x grid_w grid of rows, S = (f x f block mean of E) * f^2,
 *                                 out[b, n, c] = E[map[n]] * (lr[b, block(map[n]), c] * (1 / S[block(map[n])])); lr then holds
 *                                 (grid_h / f) * (grid_w / f) rows per sample
 * hr = [batch, cells, channels] rows ld_hr floats apart, lr the same with ld_lr (lr may be the forecaster's input rows: ld_lr =
 * feature_dim + aux_dim); inv_ptr[cells + 1] / inv_idx[nodes] = CSR of map's inverse (row k -> the nodes reading it, ascending).
 * map values must lie in [0, cells): they are not checked on the device.  The statistics are reduced in one fixed order
 * (fp64 partials per slab of rows, no atomics): results are bitwise reproducible.  More than 2^31-1 elements in any
 * operand: GW_E_UNSUPPORTED. */
#define GW_CONSTRAINT_ADDITIVE 1
#define GW_CONSTRAINT_MULTIPLICATIVE 2
#define GW_CONSTRAINT_SOFTMAX 3
typedef struct gw_constraint_args {
  int32_t type;        /* GW_CONSTRAINT_* */
  int32_t batch, nodes, channels, cells;
  int32_t f;           /* softmax block size (upsampling_factor); 1 for the other types */
  int32_t grid_h, grid_w; /* f > 1: grid_h * grid_w == cells, both multiples of f */
  int32_t graph_rows;  /* 1: hr rows are graph nodes (3-D layer input): rows no node reads get a zero gradient */
  float exp_factor;
  const float* hr;
  int32_t ld_hr;
  const float* lr;
  int32_t ld_lr;
  const int32_t* map;
  const int32_t* inv_ptr;
  const int32_t* inv_idx;
} gw_constraint_args;
/* Workspace both calls need (0 for the softmax with f = 1; 0 with the error set on bad arguments). */
size_t gw_constraint_workspace_bytes(const gw_constraint_args* a);
/* out[b, n, :channels] (row stride ld_out); out must not alias hr or lr. */
int gw_constraint_forward(const gw_constraint_args* a, void* workspace, size_t workspace_bytes, float* out, int32_t ld_out,
                          void* stream);
/* Gradients for dout [batch, nodes, channels] (ld_dout): dhr [batch, cells, :channels] is written in full (rows no node reads:
 * zero, except the softmax on a dense 4-D grid, which like the reference computes them from a zero gradient); dlr rows
 * [batch, lr rows, :channels] are written, other columns of dlr are not touched.  Either output may be NULL. */
int gw_constraint_backward(const gw_constraint_args* a, const float* dout, int32_t ld_dout, void* workspace, size_t workspace_bytes,
                           float* dhr, int32_t ld_dhr, float* dlr, int32_t ld_dlr, void* stream);

/* =====================================================================================================================
 * ThermalizerLayer / AdaptiveUNet (graph_weather/models/layers/thermalizer.py), csrc/gw_thermal.hip.  Activations are NHWC
 * pixel rows: row (b * H + y) * W + x of an image batch, `channels` floats, row stride ld.  Everything is fp32.
 *
 * gw_thermal_conv_forward is an implicit GEMM on v_mfma_f32_16x16x4_f32 over GEMM pixels q = (b, qy, qx) of a q_h x q_w
 * grid per image:
 *   out[b, out_scale * q + out_off, co] = bias[co] + sum over live taps (ty, tx) and ci < cin of
 *                                         A(b, in_scale * q + in_off(ty, tx), ci) * w[wy * w_stride_y + wx * w_stride_x
 *                                                                                   + ci * w_stride_ci + co * w_stride_co]
 * with (wy, wx) = the taps' w_idx.  Input pixels outside in_h x in_w read zero.  One mapping serves Conv2d (stride 1), its
 * input gradient (flipped, transposed weight strides), the four output-parity sub-convolutions of
 * ConvTranspose2d(3, stride 2, pad 1, output_padding 1) and that transpose's input gradient (in_scale 2).  Taps that can
 * never hit the image are left out of the lists by the caller.
 *   a_mode GW_THERMAL_A_PLAIN    A = a[row * ld_a + ci]
 *          GW_THERMAL_A_GN_RELU  A = max(a * a_scale[b, ci] + a_shift[b, ci], 0)   (GroupNorm + ReLU on load)
 *          GW_THERMAL_A_DIFFUSE  A = sa * x + s1 * eps for ci < features (x = a rows, eps [rows, features] dense),
 *                                ci == features: x-coordinate linspace(0, 1, in_w), ci == features + 1: linspace(0, 1, in_h)
 *   e_mode GW_THERMAL_E_STORE    out[row * ld_out + co] = acc + bias
 *          GW_THERMAL_E_DIFFUSE  out[row * ld_out + co] = (noisy - s1 * (acc + bias)) / sa, noisy = sa * x + s1 * eps from
 *                                x [row * ld_x + co] and eps [row * features + co]
 * gw_thermal_conv_wgrad reads the same arguments with `out` as the output gradient G and writes
 *   dw[wy, wx, ci, co] (through the w strides) = sum_q A(q, tap, ci) * G(out pixel of q, co)
 * for the live taps only (dead taps keep what dw held), by per-tap TN products over fixed pixel slabs whose partials are
 * summed in one fixed order: bitwise reproducible, no atomics. */
#define GW_THERMAL_MAX_TAPS 7
#define GW_THERMAL_A_PLAIN 0
#define GW_THERMAL_A_GN_RELU 1
#define GW_THERMAL_A_DIFFUSE 2
#define GW_THERMAL_E_STORE 0
#define GW_THERMAL_E_DIFFUSE 1
typedef struct gw_thermal_taps {
  int32_t n;                              /* live taps along this axis, 1..GW_THERMAL_MAX_TAPS */
  int32_t in_off[GW_THERMAL_MAX_TAPS];    /* input coordinate = in_scale * q + in_off[t] */
  int32_t w_idx[GW_THERMAL_MAX_TAPS];     /* weight index of tap t along this axis */
} gw_thermal_taps;
typedef struct gw_thermal_conv_args {
  int32_t batch, in_h, in_w, out_h, out_w, q_h, q_w;
  int32_t in_scale_h, in_scale_w, out_scale_h, out_scale_w, out_off_h, out_off_w;
  gw_thermal_taps ty, tx;
  int32_t cin, cout;
  int32_t a_mode, e_mode;
  const float* a;
  int32_t ld_a, features;                 /* features: the diffusion modes' F */
  const float* a_scale;                   /* [batch, cin] (GN_RELU) */
  const float* a_shift;
  const float* w;
  int64_t w_stride_y, w_stride_x, w_stride_ci, w_stride_co;
  const float* bias;                      /* [cout] or NULL */
  float* out;
  int32_t ld_out, ld_x;
  const float* x;                         /* E_DIFFUSE: the clean rows */
  const float* eps;                       /* diffusion modes: the noise rows [rows, features] */
  float sa, s1;                           /* sqrt(alpha_bar_t), sqrt(1 - alpha_bar_t) */
} gw_thermal_conv_args;
int gw_thermal_conv_forward(const gw_thermal_conv_args* a, void* stream);
size_t gw_thermal_conv_wgrad_workspace_bytes(const gw_thermal_conv_args* a);
int gw_thermal_conv_wgrad(const gw_thermal_conv_args* a, void* workspace, size_t workspace_bytes, float* dw, void* stream);
/* out[c] = sum over rows of g[r * ld + c] (bias gradients), slab partials summed in one fixed order. */
size_t gw_thermal_colsum_workspace_bytes(int64_t rows, int32_t cols);
int gw_thermal_colsum(int64_t rows, int32_t cols, const float* g, int32_t ld, void* workspace, size_t workspace_bytes, float* out,
                      void* stream);
/* GroupNorm(groups, channels) over images of hw pixels.  Statistics: per-slab (count, mean, M2) partials merged in one fixed
 * order (Chan); stats[b, g] = (mean, rstd); scale / shift [batch, channels] = the affine the consumer applies on load
 * (gamma * rstd, beta - mean * gamma * rstd).  The backward takes dy = the gradient of relu(GroupNorm(x)) and writes dx
 * [rows, channels] dense, dgamma and dbeta. */
size_t gw_thermal_groupnorm_workspace_bytes(int32_t batch, int32_t hw, int32_t channels, int32_t groups);
int gw_thermal_groupnorm_forward(int32_t batch, int32_t hw, int32_t channels, int32_t groups, const float* x, int32_t ld_x,
                                 const float* gamma, const float* beta, float eps, void* workspace, size_t workspace_bytes,
                                 float* stats, float* scale, float* shift, void* stream);
int gw_thermal_groupnorm_backward(int32_t batch, int32_t hw, int32_t channels, int32_t groups, const float* x, int32_t ld_x,
                                  const float* scale, const float* shift, const float* stats, const float* gamma, const float* dy,
                                  int32_t ld_dy, void* workspace, size_t workspace_bytes, float* dx, float* dgamma, float* dbeta,
                                  void* stream);
/* MaxPool2d(3, 2, 1) of relu(x * scale + shift) (scale / shift [batch, channels]) -> out rows (ld_out) and the argmax
 * (pixel index y * w + x inside the image, first maximum in window order) idx [out rows, channels].  The backward gathers
 * (g1 + g2) (g2 may be NULL) at each input pixel from the <= 2 x 2 windows that hold it -> dx [rows, channels] dense. */
int gw_thermal_maxpool_forward(int32_t batch, int32_t h, int32_t w, int32_t channels, const float* x, int32_t ld_x,
                               const float* scale, const float* shift, float* out, int32_t ld_out, int32_t* idx, void* stream);
int gw_thermal_maxpool_backward(int32_t batch, int32_t h, int32_t w, int32_t channels, const int32_t* idx, const float* g1,
                                int32_t ld_g1, const float* g2, int32_t ld_g2, float* dx, void* stream);
/* Bilinear resize (interpolate(mode="bilinear", align_corners=False)) of h_in x w_in images to h_out x w_out; the backward is
 * a gather over the output pixels that read each input pixel (no atomics) -> dx [rows_in, channels] dense. */
int gw_thermal_resize_forward(int32_t batch, int32_t h_in, int32_t w_in, int32_t h_out, int32_t w_out, int32_t channels,
                              const float* x, int32_t ld_x, float* out, int32_t ld_out, void* stream);
int gw_thermal_resize_backward(int32_t batch, int32_t h_in, int32_t w_in, int32_t h_out, int32_t w_out, int32_t channels,
                               const float* g, int32_t ld_g, float* dx, void* stream);
/* Row-wise ends of the diffusion step, over rows x features:
 *   GW_THERMAL_ROWS_FINALIZE  out = (sa * p + s1 * q - s1 * r) / sa   (p = x rows, q = eps rows, r = predicted noise rows)
 *   GW_THERMAL_ROWS_SCALE     out = sa * p                            (sa carries the factor)
 *   GW_THERMAL_ROWS_AXPY      out = p + sa * q */
#define GW_THERMAL_ROWS_FINALIZE 0
#define GW_THERMAL_ROWS_SCALE 1
#define GW_THERMAL_ROWS_AXPY 2
int gw_thermal_rows(int32_t mode, int64_t rows, int32_t features, float sa, float s1, const float* p, int32_t ld_p, const float* q,
                    int32_t ld_q, const float* r, int32_t ld_r, float* out, int32_t ld_out, void* stream);

/* =====================================================================================================================
 * AMSENormalizedLoss (graph_weather/models/losses.py:98-195), csrc/gw_sht.hip: the orthonormal real spherical-harmonic
 * transform on the equiangular grid (nlat Clenshaw-Curtis latitudes with both poles, nlon longitudes) as two dense fp32
 * MFMA products with the loss fused behind the second.  lmax = nlat, mmax = min(nlat, nlon / 2 + 1) = gw_amse_mmax.
 * pred / target are `fields` = B * C dense [nlat, nlon] images each (field n has channel n % channels).  Host-built tables:
 *   dft       [gw_amse_dft_rows, nlon]: row c * rows / 2 + m holds (2 pi / nlon) * cos(2 pi m j / nlon) for c = 0 and
 *             -(2 pi / nlon) * sin(...) for c = 1, m < mmax; the other rows are zero
 *   legendre  gw_amse_legendre_floats floats: order m starts at (m * lmax - m (m - 1) / 2) * nlat and holds the rows
 *             l = m .. lmax - 1 of Pbar_l^m(cos theta_k) * w_k, nlat floats each (degrees l < m are not stored)
 * gw_amse_forward writes the scalar loss.  With coeff / gfac given (both or neither) it also saves what the backward reads:
 *   coeff [4, mmax, lmax, fields]  pred re, pred im, target re, target im of a[n, l, m]; entries with l < m are not written
 *   gfac  [2, lmax, fields]        d term / d pp and d term / d num, times 1 / (fields * (variance + epsilon))
 * gw_amse_backward writes dpred [fields, nlat, nlon] = dloss[0] * d loss / d pred.  The per-(n, l) sums and the loss terms
 * are combined in fp64 in one fixed order; no atomics, no host synchronisation.  The queries need no GPU. */
int32_t gw_amse_mmax(int32_t nlat, int32_t nlon);
int32_t gw_amse_dft_rows(int32_t nlat, int32_t nlon);
size_t gw_amse_legendre_floats(int32_t nlat, int32_t nlon);
size_t gw_amse_coeff_floats(int32_t fields, int32_t nlat, int32_t nlon);
/* backward = 0: bytes gw_amse_forward needs, else gw_amse_backward (0 with the error set on bad arguments). */
size_t gw_amse_workspace_bytes(int32_t fields, int32_t nlat, int32_t nlon, int32_t backward);
int gw_amse_forward(int32_t fields, int32_t channels, int32_t nlat, int32_t nlon, const float* pred, const float* target,
                    const float* dft, const float* legendre, const float* variance, double epsilon, void* workspace,
                    size_t workspace_bytes, float* coeff, float* gfac, float* loss, void* stream);
int gw_amse_backward(int32_t fields, int32_t nlat, int32_t nlon, const float* coeff, const float* gfac, const float* dloss,
                     const float* dft, const float* legendre, void* workspace, size_t workspace_bytes, float* dpred, void* stream);

/* The inverse transform, csrc/gw_sht.hip: torch_harmonics.InverseRealSHT(nlat, nlon, lmax, mmax = lmax + 1, grid="equiangular")
 * on the two grids GenCast's generate_isotropic_noise accepts, lmax = gw_isht_lmax: nlat when nlon = 2 nlat, nlat - 1 when
 * nlon = 2 (nlat - 1), 0 for any other shape.
 *   coeffs     interleaved complex64 [fields, lmax, mmax] (what torch.view_as_real shows).  The imaginary parts of the orders
 *              m = 0 and m = nlon / 2 are ignored, as irfft ignores them.
 *   synthesis  [2 Mp, nlon], Mp = mmax rounded up to 64: row c * Mp + m holds w_m cos(2 pi m j / nlon) for c = 0 and
 *              -w_m sin(...) for c = 1, w_0 = w_{nlon / 2} = 1 and w_m = 2 otherwise; the other rows are zero
 *   legendre   gw_isht_legendre_floats floats: order m starts at (m * lmax - m (m - 1) / 2) * nlat and holds the rows
 *              l = m .. lmax - 1 of Pbar_l^m(cos theta_k), nlat floats each (no quadrature weights)
 * out [fields / channels, nlon, nlat, channels] = scale * the transform of field b * channels + ch, written in that layout
 * directly.  One fixed summation order per element whatever the number of fields; no atomics, no host synchronisation.  The
 * queries need no GPU (gw_isht_workspace_bytes: 0 with the error set on bad arguments). */
int32_t gw_isht_lmax(int32_t nlat, int32_t nlon);
size_t gw_isht_legendre_floats(int32_t nlat, int32_t nlon);
size_t gw_isht_workspace_bytes(int32_t fields, int32_t nlat, int32_t nlon);
int gw_isht_forward(int32_t fields, int32_t channels, int32_t nlat, int32_t nlon, const float* coeffs, const float* synthesis,
                    const float* legendre, float scale, void* workspace, size_t workspace_bytes, float* out, void* stream);

/* =====================================================================================================================
 * Per-channel modulation of [B, C, *spatial] activations, csrc/gw_modulate.hip: StochasticDecompositionLayer
 * (graph_weather/models/layers/stochastic_decomposition.py) and FiLMApplier (layers/film.py).  A tensor is `rows` = B * C
 * dense rows of `spatial` floats; row r has channel r % channels.  One streaming pass each way, no atomics, no host
 * synchronisation; reductions run in one fixed order (bitwise reproducible).
 *
 * The noise eps(key, i) is a pure function of a 64-bit key (two 32-bit words in DEVICE memory, low word first; never read
 * on the host) and the flat element index i - not of launch geometry or vector width:
 *   (w0, w1, w2, w3) = Philox4x32-10(counter = (lo32(i / 4), hi32(i / 4), 0, 0), key) serve elements 4j .. 4j + 3;
 *   u = ((w >> 8) + 0.5) * 2^-24;  r = sqrt(-2 ln u_a);  even element r cos(2 pi u_b), odd element r sin(2 pi u_b)
 *   with (a, b) = (w0, w1) and (w2, w3).  u >= 2^-25, so |eps| <= sqrt(50 ln 2) = 5.89: the normal tail beyond is cut
 *   (probability 4e-9 per element).
 * gw_sdl_forward: out = x + (alpha[c] * style[r]) * e with e = noise[i] if noise is given, else eps(key, i) (x NULL with
 * alpha and style NULL: out = e, the raw noise).  gw_sdl_backward (the gradient of x is dy itself): with
 * R[r] = sum_s dy[r, s] * e, d_style[r] = alpha[c] * R[r] and d_alpha[c] = sum_b style[b, c] * R[b, c] (either may be NULL);
 * e is regenerated from the key, nothing of the size of x is kept.
 * gw_film_forward: out = x * gamma[r] + beta[r].  gw_film_backward: dx = dy * gamma[r] (needs gamma), d_gamma[r] =
 * sum_s dy * x (needs x), d_beta[r] = sum_s dy; each output may be NULL.
 * Both backwards take gw_modulate_workspace_bytes(rows, spatial) bytes of scratch (a host-side query). */
size_t gw_modulate_workspace_bytes(int64_t rows, int64_t spatial);
int gw_sdl_forward(int64_t rows, int32_t channels, int64_t spatial, const float* x, const float* style, const float* alpha,
                   const uint32_t* key, const float* noise, float* out, void* stream);
int gw_sdl_backward(int64_t rows, int32_t channels, int64_t spatial, const float* dy, const float* style, const float* alpha,
                    const uint32_t* key, const float* noise, void* workspace, size_t workspace_bytes, float* d_style,
                    float* d_alpha, void* stream);
int gw_film_forward(int64_t rows, int64_t spatial, const float* x, const float* gamma, const float* beta, float* out, void* stream);
int gw_film_backward(int64_t rows, int64_t spatial, const float* dy, const float* x, const float* gamma, void* workspace,
                     size_t workspace_bytes, float* dx, float* d_gamma, float* d_beta, void* stream);

/* =====================================================================================================================
 * FengWu-GHR (graph_weather/models/fengwu_ghr/layers.py), csrc/gw_fengwu.hip: softmax attention, knn_interpolate and the
 * exact GELU.  fp32 only; no atomics, no host synchronisation, every sum in one fixed order (bitwise reproducible).
 *
 * Attention: out[b, i, h, :] = sum_j softmax_j(scale * q[b, i, h, :] . k[b, j, h, :]) v[b, j, h, :] for `batch` x `heads`
 * independent pairs of `n` rows and `dim_head` <= 128 features (GW_E_UNSUPPORTED above).  q, k, v are read in place: row
 * (b, i) of head h starts at x + (b * n + i) * ld_qkv + h * dim_head - three column blocks of the [batch * n, 3 * heads *
 * dim_head] output of to_qkv, for instance.  out [batch * n, heads * dim_head] (leading dimension ld_out) is in the
 * "b n (h d)" order; lse [2, batch * heads, n] receives the log-sum-exp of every score row in two parts whose sum it is:
 * plane 0 the row maximum m of the scaled scores, plane 1 log sum_j exp(s_j - m) (kept apart because one fp32 of the sum
 * would carry 4e-6 of rounding into every recomputed probability at scores of 100).  The n x n scores are never written
 * (online softmax); n <= 16 runs one pair per wave, four per workgroup.
 * gw_attention_backward recomputes the probabilities from q, k and lse: delta [batch * heads, n] (scratch the caller
 * provides) = rowsum(dout * out), then one launch over key blocks writes dk and dv and one over query blocks dq, all laid
 * out like q, k, v with leading dimension ld_dqkv. */
int gw_attention_forward(int32_t batch, int32_t heads, int32_t n, int32_t dim_head, const float* q, const float* k, const float* v,
                         int32_t ld_qkv, float scale, float* out, int32_t ld_out, float* lse, void* stream);
int gw_attention_backward(int32_t batch, int32_t heads, int32_t n, int32_t dim_head, const float* q, const float* k, const float* v,
                          int32_t ld_qkv, float scale, const float* out, int32_t ld_out, const float* dout, int32_t ld_dout,
                          const float* lse, float* delta, float* dq, float* dk, float* dv, int32_t ld_dqkv, void* stream);
/* The same kernels on sequences that lie along one axis of a grid (CaFA's axial attention, graph_weather/models/cafa/
 * factorize.py), without a transposing copy: `outer` x `inner` sequences of n tokens; token i of head h of sequence (o, s)
 * starts at x + o * stride[0] + s * stride[1] + i * stride[2] + h * dim_head (strides in floats, three per operand group:
 * q / k / v, out, dout, dq / dk / dv).  For a [B, H, W, 3 * heads * dim_head] projection with row stride ld the width axis is
 * outer = B, inner = H, n = W, stride = (H W ld, W ld, ld) and the height axis outer = B, inner = W, n = H, stride =
 * (H W ld, ld, W ld).  lse [2, pairs, n] and delta [pairs, n] are dense with pairs = outer * inner * heads ordered (o, s, h).
 * gw_attention_forward / _backward are the case inner = 1, stride = (n ld, 0, ld).  dim_head > 128 is GW_E_BADARG here. */
int gw_attention_axial_forward(int32_t outer, int32_t inner, int32_t heads, int32_t n, int32_t dim_head, const float* q, const float* k,
                               const float* v, const int64_t* stride_qkv, float scale, float* out, const int64_t* stride_out, float* lse,
                               void* stream);
int gw_attention_axial_backward(int32_t outer, int32_t inner, int32_t heads, int32_t n, int32_t dim_head, const float* q, const float* k,
                                const float* v, const int64_t* stride_qkv, float scale, const float* out, const int64_t* stride_out,
                                const float* dout, const int64_t* stride_dout, const float* lse, float* delta, float* dq, float* dk,
                                float* dv, const int64_t* stride_dqkv, void* stream);
/* knn_interpolate: y[b, t, c] = sum_j w[t, j] * x[b, idx[t, j], c] / sum_j w[t, j] over the k neighbours of target t
 * (idx, w: [n_tgt, k], built on the host).  Element (b, row, c) of x / y lies at b * stride_b + row * stride_row + c *
 * stride_c floats, so [B, n, c] rows and [B, c, h, w] images are used as they lie.  The backward walks the CSR of the
 * transposed assignment: source s owns entries src_ptr[s] .. src_ptr[s + 1] - 1, entry e pointing at target src_tgt[e] with
 * weight src_w[e] = w / (sum of that target's weights); dx[b, s, c] = sum_e src_w[e] * dy[b, src_tgt[e], c]. */
int gw_knn_interpolate_forward(int32_t batch, int32_t n_tgt, int32_t channels, int32_t k, const int32_t* idx, const float* w,
                               const float* x, int64_t x_stride_b, int64_t x_stride_row, int64_t x_stride_c, float* y,
                               int64_t y_stride_b, int64_t y_stride_row, int64_t y_stride_c, void* stream);
int gw_knn_interpolate_backward(int32_t batch, int32_t n_src, int32_t channels, const int32_t* src_ptr, const int32_t* src_tgt,
                                const float* src_w, const float* dy, int64_t y_stride_b, int64_t y_stride_row, int64_t y_stride_c,
                                float* dx, int64_t x_stride_b, int64_t x_stride_row, int64_t x_stride_c, void* stream);
/* y = x * Phi(x) with the exact (erf) normal CDF, on n dense floats; dx = dy * (Phi(x) + x * phi(x)). */
int gw_gelu_forward(int64_t n, const float* x, float* y, void* stream);
int gw_gelu_backward(int64_t n, const float* x, const float* dy, float* dx, void* stream);


/* =====================================================================================================================
 * CaFA (graph_weather/models/cafa), csrc/gw_cafa.hip: the patch convolutions as fp32 MFMA products over the patch view of
 * an NCHW image [batch, channels, h, w] read or written as it lies: oh = ceil(h / f), ow = ceil(w / f) patches per image,
 * row m = (b, py, px) of the channels-last rows, k = (c, ky, kx) of the weight [dim, channels * f * f] (Conv2d's
 * [dim, channels, f, f] and ConvTranspose2d's [dim, channels, f, f] alike).  Pixels past h or w read as zero and are never
 * written.  No atomics, no host synchronisation; the weight and bias gradients are per-slab partials (1024 patches each)
 * added in slab order, in gw_patch_workspace_bytes (a host-side query; 0 with the error set on bad arguments) of scratch.
 *   gw_patch_embed_forward    out[m, :dim] = bias + weight . patch(x, m)                              (Conv2d, kernel = stride = f)
 *   gw_patch_embed_backward   dx (may be NULL), dweight and dbias (both or neither) from dout [rows, dim]
 *   gw_patch_expand_forward   out[b, c, f py + ky, f px + kx] = bias[c] + sum_d rows[m, d] weight[d, (c, ky, kx)]   (ConvTranspose2d)
 *   gw_patch_expand_backward  d_rows (may be NULL), dweight and dbias (both or neither) from dout [batch, channels, h, w] */
size_t gw_patch_workspace_bytes(int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t f, int32_t dim);
int gw_patch_embed_forward(int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t f, int32_t dim, const float* x,
                           const float* weight, const float* bias, float* out, int32_t ld_out, void* stream);
int gw_patch_embed_backward(int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t f, int32_t dim, const float* x,
                            const float* weight, const float* dout, int32_t ld_dout, void* workspace, size_t workspace_bytes,
                            float* dx, float* dweight, float* dbias, void* stream);
int gw_patch_expand_forward(int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t f, int32_t dim, const float* rows,
                            int32_t ld_rows, const float* weight, const float* bias, float* out, void* stream);
int gw_patch_expand_backward(int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t f, int32_t dim, const float* rows,
                             int32_t ld_rows, const float* weight, const float* dout, void* workspace, size_t workspace_bytes,
                             float* d_rows, int32_t ld_drows, float* dweight, float* dbias, void* stream);

/* =====================================================================================================================
 * Aurora (graph_weather/models/aurora), csrc/gw_aurora.hip and the MASKED attention kernels of csrc/gw_fengwu.hip.
 * All fp32, no atomics, every sum in one fixed order (bitwise reproducible), no host synchronisation.
 *
 * Key-padding masks: gw_attention_axial_forward / _backward with key_bias [outer * inner, n] added to the scaled scores of
 * every head and query of a sequence - 0 keeps a key, -inf drops it.  A leading run of dropped keys leaves the online softmax
 * at (maximum, sum, output) = (-inf, 0, 0) without NaN; dk and dv of a dropped key are exactly zero; an all-zero bias gives the
 * bits of the unmasked entry points.  A sequence whose keys are all dropped is NaN, as in torch. */
int gw_attention_masked_forward(int32_t outer, int32_t inner, int32_t heads, int32_t n, int32_t dim_head, const float* q, const float* k,
                                const float* v, const int64_t* stride_qkv, const float* key_bias, float scale, float* out,
                                const int64_t* stride_out, float* lse, void* stream);
int gw_attention_masked_backward(int32_t outer, int32_t inner, int32_t heads, int32_t n, int32_t dim_head, const float* q, const float* k,
                                 const float* v, const int64_t* stride_qkv, const float* key_bias, float scale, const float* out,
                                 const int64_t* stride_out, const float* dout, const int64_t* stride_dout, const float* lse, float* delta,
                                 float* dq, float* dk, float* dv, const int64_t* stride_dqkv, void* stream);
/* EarthSystemLoss (model.py): pred, target [batch, n, channels], points [batch, n, 2] (longitude, latitude in degrees), dense.
 *   mse       mean (pred - target)^2                                   (target NULL: 0)
 *   spatial   mean over [n, n, channels] of m_ij ((pred_i - target_i) - (pred_j - target_j))^2, m_ij = 1 where points i and j
 *             are closer than 5 degrees; `spatial` != 0 asks for it and needs batch == 1 (the reference cannot form it
 *             otherwise) and channels <= 128 (GW_E_UNSUPPORTED above); pairs are walked in tiles, nothing n x n is written.
 *             pair_rows [n, channels] receives G_i = sum_j m_ij (e_i - e_j): the gradient is 4 G / (n^2 channels).
 *   physical  mean relu(-pred) + mean relu(pred - 500) + 0.1 mean_r relu(pred[r, 0] - (1 - |lat_r| / 90) mean(pred))
 *   total     alpha mse + beta spatial + gamma physical
 * out = (total, mse, spatial, physical); stats [2] is kept for the backward (the mean of pred and the sum of the active
 * latitude weights).  workspace: gw_earth_loss_workspace_bytes (host-side query, 0 with the error set on bad arguments), 8-byte
 * aligned: per-workgroup fp64 partials added in workgroup order.
 * gw_earth_loss_backward: gout [4] = upstream gradients of the four scalars (on the device); dpred and / or dtarget. */
size_t gw_earth_loss_workspace_bytes(int32_t batch, int32_t n, int32_t channels);
int gw_earth_loss_forward(int32_t batch, int32_t n, int32_t channels, const float* pred, const float* target, const float* points,
                          int32_t spatial, float alpha, float beta, float gamma, void* workspace, size_t workspace_bytes, float* out,
                          float* pair_rows, float* stats, void* stream);
int gw_earth_loss_backward(int32_t batch, int32_t n, int32_t channels, const float* pred, const float* target, const float* points,
                           int32_t spatial, float alpha, float beta, float gamma, const float* pair_rows, const float* stats,
                           const float* gout, float* dpred, float* dtarget, void* stream);
/* out[b, :width] = mean over the `tokens` rows of sample b of x [batch * tokens, width]; dx[(b, s)] = dout[b] / tokens. */
int gw_token_mean_forward(int32_t batch, int32_t tokens, int32_t width, const float* x, int32_t ld_x, float* out, int32_t ld_out,
                          void* stream);
int gw_token_mean_backward(int32_t batch, int32_t tokens, int32_t width, const float* dout, int32_t ld_dout, float* dx, int32_t ld_dx,
                           void* stream);
/* y = max(x, 0) on n floats (its gradient is gw_relu_backward on the output). */
int gw_relu_forward(int64_t n, const float* x, float* y, void* stream);
/* out[r, :width] = x[r, :width] * row_factor[r] (a per-point mask; its gradient is the same call on dout). */
int gw_row_scale(int64_t rows, int32_t width, const float* x, int32_t ld_x, const float* row_factor, float* out, int32_t ld_out,
                 void* stream);
/* Weight gradients in one fixed order (the training kernels above add their row slabs with float atomics): per-slab partials in the
 * caller's workspace (the *_workspace_bytes queries are host side; 0 with the error set on bad arguments), added in slab order.
 *   gw_gemm_tn_ordered              c[i, j] = sum_r a[r, i] b[r, j] (c [m, n] is overwritten), colsum[i] = sum_r a[r, i] (may be NULL)
 *   gw_layernorm_backward_ordered   gw_layernorm_backward (eps 1e-5, width <= 4096) with dgamma and dbeta overwritten */
size_t gw_gemm_tn_ordered_workspace_bytes(int32_t m, int32_t n, int64_t rows);
int gw_gemm_tn_ordered(int32_t m, int32_t n, int64_t rows, const float* a, int32_t lda, const float* b, int32_t ldb, void* workspace,
                       size_t workspace_bytes, float* c, int32_t ldc, float* colsum, void* stream);
size_t gw_layernorm_backward_ordered_workspace_bytes(int64_t rows, int32_t width);
int gw_layernorm_backward_ordered(int64_t rows, int32_t width, const float* dn, int32_t ld_dn, const float* y, int32_t ld_y,
                                  const float* gamma, void* workspace, size_t workspace_bytes, float* dy, int32_t ld_dy, float* dgamma,
                                  float* dbeta, void* stream);
/* 3 x 3 x 3 convolutions, stride 1, padding 1 (csrc/gw_conv3d.hip): implicit GEMMs on fp32 MFMA, the zero padding a bounds
 * predicate.  A volume [batch, channels, d, h, w] is addressed by three strides in floats - element (b, c, v = (z h + y) w + x)
 * at b s[0] + c s[1] + v s[2] - so NCDHW tensors (c d h w, d h w, 1) and channels-last rows [(b, v), c] (d h w ld, 1, ld) are
 * read and written as they lie.  x has cin channels, out cout.
 *   transposed 0  nn.Conv3d: weight [cout, cin, 3, 3, 3];   transposed 1  nn.ConvTranspose3d: weight [cin, cout, 3, 3, 3]
 * bias [cout] may be NULL.  gw_conv3d_backward: dx (may be NULL; laid out by stride_dx), dweight and dbias (both or neither).
 * The weight and bias gradients are partials per slab of 1024 voxels in gw_conv3d_workspace_bytes (host-side query, 0 with the
 * error set on bad arguments) of scratch, added in slab order: no atomics, bitwise reproducible. */
size_t gw_conv3d_workspace_bytes(int32_t batch, int32_t cin, int32_t cout, int32_t d, int32_t h, int32_t w, int32_t transposed);
int gw_conv3d_forward(int32_t batch, int32_t cin, int32_t cout, int32_t d, int32_t h, int32_t w, int32_t transposed, const float* x,
                      const int64_t* stride_x, const float* weight, const float* bias, float* out, const int64_t* stride_out,
                      void* stream);
int gw_conv3d_backward(int32_t batch, int32_t cin, int32_t cout, int32_t d, int32_t h, int32_t w, int32_t transposed, const float* x,
                       const int64_t* stride_x, const float* weight, const float* dout, const int64_t* stride_dout, void* workspace,
                       size_t workspace_bytes, float* dx, const int64_t* stride_dx, float* dweight, float* dbias, void* stream);

/* The convolution towers of WeatherMesh (csrc/gw_convnd.hip; graph_weather/models/weathermesh/layers.py): convolutions with
 * kernel 1 or 3, padding k / 2 and stride 1 or 2 per axis, BatchNorm statistics, the residual tail gelu(bn2(y2) + bn_skip(ys)) and
 * 2 x bilinear upsampling.  fp32, no atomics, every launch bitwise repeatable.  Volumes are addressed by three strides as above.
 *
 * geo[12] = batch, cin, cout, d, h, w (of the convolution's INPUT), kd, kh, kw (1 or 3), sd, sh, sw (1 or 2); the output has
 * (L - 1) / s + 1 voxels per axis; a 2-D convolution is d = kd = sd = 1.  weight [cout, cin, kd, kh, kw] contiguous.
 *   gw_convnd_forward   out = bias + conv(A(x)); a_mode PLAIN: A(x) = x; BN_GELU: A(x) = gelu(x a_scale[c] + a_shift[c]) (exact
 *                       erf form), applied on load before the zero padding; bias [cout] may be NULL.
 *   gw_convnd_dgrad     dx (the input's layout) = the data gradient of dout (the output's), one launch per parity class of the
 *                       strided axes with that class's own taps; accumulate != 0: dx += it.
 *   gw_convnd_wgrad     dweight and dbias (may be NULL) from A(x) and dout: partials per slab of 1024 output voxels in
 *                       gw_convnd_workspace_bytes (host-side query, 0 with the error set on bad arguments), added in slab order.
 * gw_convnd_bn_stats: the table stats [4][channels] = scale (gamma rstd), shift (beta - mean scale), mean, rstd of a BatchNorm
 *   over (batch, voxels) of x.  training != 0: batch mean and biased variance (two passes, one workgroup per channel) and, when
 *   the running buffers are given, running = (1 - momentum) running + momentum (mean | unbiased variance); training == 0: mean and
 *   variance are the running buffers' and x is not read.
 * gw_convnd_tail_forward: out = gelu(y2 scale2 + shift2 + ys scales + shifts) from the tables st2 and sts; ys NULL: one term.
 * gw_convnd_tail_backward: dz = dout gelu'(.) is recomputed; one reduction launch writes sums [4][channels] = sum dz, sum dz zhat2,
 *   sum dz, sum dz zhats (d beta and d gamma of the two norms; rows 0 and 1 only when ys is NULL), one apply launch writes
 *   dy2 = scale2 (dz - mean dz - zhat2 mean(dz zhat2)) (training) or scale2 dz (training == 0), and dys likewise.
 * gw_convnd_upsample2x: F.interpolate(scale_factor = (1, 2, 2), align_corners = False) of x [batch, channels, d, h, w] into out
 *   [.., d, 2 h, 2 w]; backward != 0: x is the gradient of the upsampled volume, out the source's (gather form). */
#define GW_CONVND_A_PLAIN 0
#define GW_CONVND_A_BN_GELU 1
size_t gw_convnd_workspace_bytes(const int32_t* geo);
int gw_convnd_forward(const int32_t* geo, int32_t a_mode, const float* x, const int64_t* stride_x, const float* a_scale,
                      const float* a_shift, const float* weight, const float* bias, float* out, const int64_t* stride_out,
                      void* stream);
int gw_convnd_dgrad(const int32_t* geo, const float* dout, const int64_t* stride_dout, const float* weight, float* dx,
                    const int64_t* stride_dx, int32_t accumulate, void* stream);
int gw_convnd_wgrad(const int32_t* geo, int32_t a_mode, const float* x, const int64_t* stride_x, const float* a_scale,
                    const float* a_shift, const float* dout, const int64_t* stride_dout, void* workspace, size_t workspace_bytes,
                    float* dweight, float* dbias, void* stream);
int gw_convnd_bn_stats(int32_t batch, int32_t channels, int64_t voxels, int32_t training, const float* x, const int64_t* stride_x,
                       const float* gamma, const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                       float* stats, void* stream);
int gw_convnd_tail_forward(int32_t batch, int32_t channels, int64_t voxels, const float* y2, const int64_t* stride_y2, const float* st2,
                           const float* ys, const int64_t* stride_ys, const float* sts, float* out, const int64_t* stride_out,
                           void* stream);
int gw_convnd_tail_backward(int32_t batch, int32_t channels, int64_t voxels, int32_t training, const float* dout,
                            const int64_t* stride_dout, const float* y2, const int64_t* stride_y2, const float* st2, const float* ys,
                            const int64_t* stride_ys, const float* sts, float* sums, float* dy2, const int64_t* stride_dy2, float* dys,
                            const int64_t* stride_dys, void* stream);
int gw_convnd_upsample2x(int32_t batch, int32_t channels, int32_t d, int32_t h, int32_t w, int32_t backward, const float* x,
                         const int64_t* stride_x, float* out, const int64_t* stride_out, void* stream);

/* =====================================================================================================================
 * GenCast layers (graph_weather/models/gencast/layers), csrc/gw_gencast.hip: graph-transformer attention (the TransformerConv
 * of the mesh processor) and the row operations around it.  All fp32, no atomics, every sum in one fixed order (bitwise
 * reproducible), no host synchronisation; a launch over 0 rows or 0 edges returns GW_OK without launching (the caller zero-fills
 * what such a launch would have written).
 *
 * Graph attention over a destination-sorted CSR (GraphPlan): the edges [dst_ptr[i], dst_ptr[i + 1]) end in destination row i,
 * sorted edge t starts in source row src[t] and is the caller's edge perm[t] (perm NULL: t).  Per head h of `heads`, with
 * C = dim_head >= 1 and heads * C <= 4096 (GW_E_UNSUPPORTED above):
 *   s_t = q[i, h] . (k[src[t], h] + e[perm[t], h]) / sqrt(C),  alpha = softmax of s over the edges of i,
 *   out[i, h] = sum_t alpha_t (v[src[t], h] + e[perm[t], h]);  a destination without edges gets 0.
 * q [n_dst, heads C] is read from the destination table, k and v [n_src, heads C] from the source table, each with its own
 * leading dimension (column blocks of one stacked projection are read in place); e [n_edges, heads C] (may be NULL) is read in
 * the caller's edge order.  mean 0: out [n_dst, heads C] holds the heads side by side; mean 1: out [n_dst, C] is their mean and
 * out_heads [n_dst, heads C] (may be NULL in inference) receives the per-head rows the backward needs.  lse [2, n_dst * heads]:
 * plane 0 the maximum of the scores of (i, h), plane 1 log sum_t exp(s_t - max) - two planes for the reason given at
 * gw_attention_forward; both 0 for a destination without edges.  The softmax is online: nothing of size E x heads x C or
 * E x heads is written.  dim_head and every leading dimension a multiple of 4 with 16-byte aligned tables: 16-byte loads;
 * anything else runs a scalar path.  One wave walks one destination's edges: any degree is correct, near-uniform degrees are fast.
 *
 * gw_graph_attention_backward recomputes the probabilities from q, k, e and lse.  out_heads: the per-head forward rows (mean 0:
 * out itself); dout [n_dst, heads C] (mean 1: [n_dst, C]).  One launch over destinations writes delta [n_dst * heads] (scratch
 * the caller provides) = rowsum(dout_h o out_h), dq and - with e - de [n_edges, heads C] in the caller's edge order (de NULL:
 * not wanted); one launch over sources walks src_pos / src_ptr (GraphPlan.src_sorted: sorted positions grouped by source row;
 * dst[t] = destination row of sorted edge t) and writes dk and dv.  Every row of dq, dk, dv, de is written. */
int gw_graph_attention_forward(int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t heads, int32_t dim_head, const int32_t* dst_ptr,
                               const int32_t* src, const int64_t* perm, const float* q, int32_t ld_q, const float* k, int32_t ld_k,
                               const float* v, int32_t ld_v, const float* e, int32_t ld_e, int32_t mean, float* out, int32_t ld_out,
                               float* out_heads, int32_t ld_out_heads, float* lse, void* stream);
int gw_graph_attention_backward(int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t heads, int32_t dim_head, const int32_t* dst_ptr,
                                const int32_t* src, const int32_t* dst, const int64_t* perm, const int32_t* src_pos,
                                const int32_t* src_ptr, const float* q, int32_t ld_q, const float* k, int32_t ld_k, const float* v,
                                int32_t ld_v, const float* e, int32_t ld_e, int32_t mean, const float* out_heads, int32_t ld_out_heads,
                                const float* dout, int32_t ld_dout, const float* lse, float* delta, float* dq, int32_t ld_dq, float* dk,
                                int32_t ld_dk, float* dv, int32_t ld_dv, float* de, int32_t ld_de, void* stream);
/* Batch-shared form: `batch` >= 1 disconnected copies of one graph (what the reference's utils/batching.py builds by replicating
 * edge_index and edge_attr) share ONE plan over n_dst, n_src and n_edges.  Copy b's rows are rows b n_dst .. of q, out, out_heads,
 * dq, dout [batch n_dst, .] and rows b n_src .. of k, v, dk, dv [batch n_src, .]; lse is [2, batch n_dst heads], delta
 * [batch n_dst heads]; all row offsets are 64-bit.  The edge tables e and de start e_batch_stride rows further per copy:
 * 0 = one table [n_edges, heads C] read by every copy, >= n_edges = one table per copy (anything between: GW_E_BADARG).  The work
 * item is (copy, destination, head) with the per-item arithmetic of the calls above: on the replicated graph they give bitwise
 * the same out, lse, dq, dk, dv.  With a shared table de [n_edges, heads C] is the sum over the copies in copy order 0, 1, ...,
 * formed by the wave that owns the destination (plain stores, no atomics).  batch = 1 is the call above. */
int gw_graph_attention_batched_forward(int32_t batch, int64_t e_batch_stride, int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t heads,
                                       int32_t dim_head, const int32_t* dst_ptr, const int32_t* src, const int64_t* perm, const float* q,
                                       int32_t ld_q, const float* k, int32_t ld_k, const float* v, int32_t ld_v, const float* e, int32_t ld_e,
                                       int32_t mean, float* out, int32_t ld_out, float* out_heads, int32_t ld_out_heads, float* lse,
                                       void* stream);
int gw_graph_attention_batched_backward(int32_t batch, int64_t e_batch_stride, int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t heads,
                                        int32_t dim_head, const int32_t* dst_ptr, const int32_t* src, const int32_t* dst,
                                        const int64_t* perm, const int32_t* src_pos, const int32_t* src_ptr, const float* q, int32_t ld_q,
                                        const float* k, int32_t ld_k, const float* v, int32_t ld_v, const float* e, int32_t ld_e,
                                        int32_t mean, const float* out_heads, int32_t ld_out_heads, const float* dout, int32_t ld_dout,
                                        const float* lse, float* delta, float* dq, int32_t ld_dq, float* dk, int32_t ld_dk, float* dv,
                                        int32_t ld_dv, float* de, int32_t ld_de, void* stream);
/* ConditionalLayerNorm (modules.py): out[r] = act(scale[r] o LN(x[r]) + bias[r]) with LN = LayerNorm without affine, eps 1e-5, and
 * scale, bias one row per row of x; act = GW_ACT_*.  Backward: dx, dscale, dbias (each may be NULL; dscale and dbias share ld_dsb). */
#define GW_ACT_NONE 0
#define GW_ACT_RELU 1
#define GW_ACT_SILU 2
int gw_cond_layernorm_forward(int64_t rows, int32_t width, int32_t act, const float* x, int32_t ld_x, const float* scale, int32_t ld_scale,
                              const float* bias, int32_t ld_bias, float* out, int32_t ld_out, void* stream);
int gw_cond_layernorm_backward(int64_t rows, int32_t width, int32_t act, const float* x, int32_t ld_x, const float* scale,
                               int32_t ld_scale, const float* bias, int32_t ld_bias, const float* dout, int32_t ld_dout, float* dx,
                               int32_t ld_dx, float* dscale, float* dbias, int32_t ld_dsb, void* stream);
/* The same with one scale and one bias row per group of rows_per_group consecutive rows (row r reads row r / rows_per_group; the
 * last group may be shorter): the noise conditioning of a batch, one row per sample.  The forward gives bitwise what the call
 * above gives on row-repeated scale and bias.  Backward: dx as above; dscale and dbias [groups, width] (each may be NULL) sum over
 * the group's rows as partials per slab of 256 rows in gw_cond_layernorm_grouped_workspace_bytes (host-side query; 0 with the
 * error set on bad arguments) of scratch, added in slab order.  At most 65535 groups and 65535 slabs per group. */
int gw_cond_layernorm_grouped_forward(int64_t rows, int32_t width, int32_t act, int64_t rows_per_group, const float* x, int32_t ld_x,
                                      const float* scale, int32_t ld_scale, const float* bias, int32_t ld_bias, float* out, int32_t ld_out,
                                      void* stream);
size_t gw_cond_layernorm_grouped_workspace_bytes(int64_t rows, int32_t width, int64_t rows_per_group);
int gw_cond_layernorm_grouped_backward(int64_t rows, int32_t width, int32_t act, int64_t rows_per_group, const float* x, int32_t ld_x,
                                       const float* scale, int32_t ld_scale, const float* bias, int32_t ld_bias, const float* dout,
                                       int32_t ld_dout, void* workspace, size_t workspace_bytes, float* dx, int32_t ld_dx, float* dscale,
                                       float* dbias, int32_t ld_dsb, void* stream);
/* The fan-out form, where one row turns into `members` conditioned rows (an ensemble: B samples x N members): x [B M, width] with
 * M = rows_per_sample (x_rows = B M), scale and bias [B N, width], out [B N M, width]; output row (b, n, m) normalises x row (b, m)
 * and applies row b N + n of scale and bias.  The statistics are formed once per x row by the wave that owns it, which writes the
 * row's N outputs; the forward gives bitwise what gw_cond_layernorm_grouped_forward gives on x repeated per member.  Backward: dout
 * [B N M, width]; dx [B M, width] is the sum over the members in member order, formed by the owning wave with plain stores; dscale
 * and dbias [B N, width] through slab partials added in slab order as above (workspace: gw_cond_layernorm_fanout_workspace_bytes).
 * No atomics.  At most 65535 (sample, member) pairs. */
int gw_cond_layernorm_fanout_forward(int64_t x_rows, int32_t width, int32_t act, int64_t rows_per_sample, int32_t members, const float* x,
                                     int32_t ld_x, const float* scale, int32_t ld_scale, const float* bias, int32_t ld_bias, float* out,
                                     int32_t ld_out, void* stream);
size_t gw_cond_layernorm_fanout_workspace_bytes(int64_t x_rows, int32_t width, int64_t rows_per_sample, int32_t members);
int gw_cond_layernorm_fanout_backward(int64_t x_rows, int32_t width, int32_t act, int64_t rows_per_sample, int32_t members, const float* x,
                                      int32_t ld_x, const float* scale, int32_t ld_scale, const float* bias, int32_t ld_bias,
                                      const float* dout, int32_t ld_dout, void* workspace, size_t workspace_bytes, float* dx, int32_t ld_dx,
                                      float* dscale, float* dbias, int32_t ld_dsb, void* stream);
/* The Denoiser's preconditioning (denoiser.py, utils/noise.py; Karras et al. 2022) on rows r = b grid_rows + g of `batch` samples,
 * sigma [batch] > 0, the coefficients formed in float32 in the reference's order of operations from sigma and d = sigma_data > 0:
 * c_in = 1 / sqrt(sigma^2 + d^2), c_skip = d^2 / (sigma^2 + d^2), c_out = sigma d / sqrt(sigma^2 + d^2), c_noise = 1/4 log sigma.
 * input_forward: out[r] = (c_in(sigma_b) z[r] | x[r] | stat[g]) of widths w_z, w_x, w_s - the encoder's grid input rows with the
 * static grid features stat [grid_rows, w_s] - and c_noise [batch] (may be NULL); input_backward: dz[r] = c_in dout[r, :w_z],
 * dx[r] = dout[r, w_z : w_z + w_x] (each may be NULL).  output_forward: out[r] = c_skip(sigma_b) z[r] + c_out(sigma_b) preds[r];
 * output_backward: dz = c_skip dout, dpreds = c_out dout (each may be NULL).  sigma itself gets no gradient. */
int gw_gencast_precond_input_forward(int32_t batch, int64_t grid_rows, int32_t w_z, int32_t w_x, int32_t w_s, float sigma_data,
                                     const float* sigma, const float* z, int32_t ld_z, const float* x, int32_t ld_x, const float* stat,
                                     int32_t ld_stat, float* out, int32_t ld_out, float* c_noise, void* stream);
int gw_gencast_precond_input_backward(int32_t batch, int64_t grid_rows, int32_t w_z, int32_t w_x, float sigma_data, const float* sigma,
                                      const float* dout, int32_t ld_dout, float* dz, int32_t ld_dz, float* dx, int32_t ld_dx,
                                      void* stream);
int gw_gencast_precond_output_forward(int32_t batch, int64_t grid_rows, int32_t width, float sigma_data, const float* sigma, const float* z,
                                      int32_t ld_z, const float* preds, int32_t ld_preds, float* out, int32_t ld_out, void* stream);
int gw_gencast_precond_output_backward(int32_t batch, int64_t grid_rows, int32_t width, float sigma_data, const float* sigma,
                                       const float* dout, int32_t ld_dout, float* dz, int32_t ld_dz, float* dpreds, int32_t ld_dpreds,
                                       void* stream);
/* The Sampler's state update (sampler.py): out = a x + b y + c z on n dense floats, host scalars.  A NULL operand is skipped (at
 * least one is required); out may alias x.  An element's value does not depend on its position or on n. */
int gw_gencast_sampler_combine(int64_t n, float a, const float* x, float b, const float* y, float c, const float* z, float* out,
                               void* stream);
/* WeightedMSELoss (weighted_mse_loss.py) on pred / target [batch, nlon, nlat, nvar] dense, sigma [batch] > 0:
 * loss = sum (pred - target)^2 aw[lat] fw[var] lambda(sigma_b) / (batch nlon nlat nvar), lambda(s) = (s^2 + d^2) / (s d)^2 with
 * d = sigma_data, area_weights [nlat] and features_weights [nvar] each optional (NULL).  Sums of slabs of 4096 elements in fp64,
 * added by one workgroup in a fixed order; no atomics.  nan_flag[0] is set to 1 when a squared residual is NaN, else to 0.
 * backward: dpred = dloss[0] * d loss / d pred.  gw_gencast_weighted_mse_workspace_bytes: host-side query (0 with the error set
 * on bad arguments). */
size_t gw_gencast_weighted_mse_workspace_bytes(int32_t batch, int32_t nlon, int32_t nlat, int32_t nvar);
int gw_gencast_weighted_mse_forward(int32_t batch, int32_t nlon, int32_t nlat, int32_t nvar, float sigma_data, const float* pred,
                                    const float* target, const float* sigma, const float* area_weights, const float* features_weights,
                                    void* workspace, size_t workspace_bytes, float* loss, int32_t* nan_flag, void* stream);
int gw_gencast_weighted_mse_backward(int32_t batch, int32_t nlon, int32_t nlat, int32_t nvar, float sigma_data, const float* pred,
                                     const float* target, const float* sigma, const float* area_weights, const float* features_weights,
                                     const float* dloss, float* dpred, void* stream);
/* TransformerConv's beta gate: g[r] = sigmoid(w_a . out[r] + w_b . x_r[r] + w_c . (out[r] - x_r[r])), w = [w_a | w_b | w_c]
 * (lin_beta.weight, 3 width floats), y[r] = g x_r[r] + (1 - g) out[r]; gate [rows] keeps g for the backward.  Backward: d_out and
 * d_xr (each may be NULL, leading dimension ld_d) and dw [3 width], formed as partials per slab of 256 rows in
 * gw_beta_gate_workspace_bytes (host-side query; 0 with the error set on bad arguments) of scratch, added in slab order. */
int gw_beta_gate_forward(int64_t rows, int32_t width, const float* out, int32_t ld_out, const float* x_r, int32_t ld_xr, const float* w,
                         float* y, int32_t ld_y, float* gate, void* stream);
size_t gw_beta_gate_workspace_bytes(int64_t rows, int32_t width);
int gw_beta_gate_backward(int64_t rows, int32_t width, const float* out, int32_t ld_out, const float* x_r, int32_t ld_xr, const float* w,
                          const float* gate, const float* dy, int32_t ld_dy, void* workspace, size_t workspace_bytes, float* d_out,
                          float* d_xr, int32_t ld_d, float* dw, void* stream);
/* y = x sigmoid(x) on n dense floats; dx = dy sigmoid(x) (1 + x (1 - sigmoid(x))). */
int gw_silu_forward(int64_t n, const float* x, float* y, void* stream);
int gw_silu_backward(int64_t n, const float* x, const float* dy, float* dx, void* stream);
/* FourierEmbedding.fourier_features (modules.py): out[r, i] = cos(t[r] f_i), out[r, F + i] = sin(t[r] f_i) for i < F =
 * num_frequencies, f_i = exp(-ln(base_period) i / F) formed in float32, accurate cosf / sinf.  Backward: dt[r]. */
int gw_fourier_forward(int64_t rows, int32_t num_frequencies, float base_period, const float* t, float* out, int32_t ld_out, void* stream);
int gw_fourier_backward(int64_t rows, int32_t num_frequencies, float base_period, const float* t, const float* dout, int32_t ld_dout,
                        float* dt, void* stream);
/* EnsembleCRPSLoss: the (almost) fair continuous ranked probability score of `members` = N ensemble members against the truth, on
 * pred [batch, N, nlon, nlat, nvar] and target [batch, nlon, nlat, nvar], dense.  Per (sample, grid point, feature)
 *   v = (1/N) sum_i |x_i - y| - 2 c2 sum_{i<j} |x_i - x_j|,  c2 = alpha / (2 N (N-1)) + (1 - alpha) / (2 N^2)  (0 at N = 1),
 * alpha in [0, 1]: 1 the fair score (needs N >= 2), 0 the plain ensemble score.  fp32 on direct differences, sum_i in member order,
 * sum_{i<j} in (i, j) order; 1/N and 2 c2 are formed in double and rounded once.  N <= 16 keeps the members in registers (each value
 * is read once); N up to 1024 re-reads them through the cache and carries the two sums in fp64.  The loss is w v, w =
 * area_weights[lat] features_weights[var] (each optional, NULL).  reduction GW_CRPS_MEAN: out[0] = mean over batch nlon nlat nvar,
 * from sums of slabs of 4096 elements of one sample in fp64, added by one workgroup in a fixed order (workspace:
 * gw_ensemble_crps_workspace_bytes = 8 batch ceil(nlon nlat nvar / 4096), a host-side query, 0 with the error set on bad arguments);
 * GW_CRPS_NONE: out [batch, nlon, nlat, nvar] = the weighted field, workspace unused (may be NULL).
 * backward: dpred = dout * d out / d pred with sign(0) = 0 (ties contribute exactly zero), dout [1] (MEAN) or the field (NONE); the
 * signs are recomputed from pred and target.  No atomics, no host reads. */
#define GW_CRPS_MEAN 0
#define GW_CRPS_NONE 1
size_t gw_ensemble_crps_workspace_bytes(int32_t batch, int32_t members, int32_t nlon, int32_t nlat, int32_t nvar);
int gw_ensemble_crps_forward(int32_t batch, int32_t members, int32_t nlon, int32_t nlat, int32_t nvar, double alpha, int32_t reduction,
                             const float* pred, const float* target, const float* area_weights, const float* features_weights,
                             void* workspace, size_t workspace_bytes, float* out, void* stream);
int gw_ensemble_crps_backward(int32_t batch, int32_t members, int32_t nlon, int32_t nlat, int32_t nvar, double alpha, int32_t reduction,
                              const float* pred, const float* target, const float* area_weights, const float* features_weights,
                              const float* dout, float* dpred, void* stream);

/* GenDA (genda/model.py of the reference): the Denoiser's preconditioning with up to two conditioning columns (sensor mask, sensor
 * values) and `copies` (1 or 2) evaluations in one pass; coefficients as for gw_gencast_precond_* above.  Source row r = b grid_rows
 * + g of `batch` samples; c0, c1: one float per source row with a row stride each, either may be NULL (n_cond = the pointers given,
 * in order).  input_forward writes (c_in(sigma_b) z[r] | x[r] | c0[r] | c1[r] | stat[g]) of widths w_z, w_x, n_cond, w_s to out row
 * r and, with copies = 2, the same with ZERO conditioning to row batch grid_rows + r (the unconditional evaluation of classifier-free
 * guidance: sample batch + b of a pass at batch 2 batch); drop = 1 writes zeros for the conditioning of copy 0 as well (the training
 * dropout, decided on the host) and reads no conditioning.  c_noise [copies batch] (may be NULL).  With copies 1 and no
 * conditioning the result is that of gw_gencast_precond_input_forward bit for bit.
 * input_backward, dout [copies batch grid_rows, >= w_z + w_x + n_cond]: dz = c_in (dout_copy0 + dout_copy1), dx = dout_copy0 +
 * dout_copy1 (copy order), dc0 / dc1 = columns w_z + w_x / + 1 of copy 0 (zeros with drop); each output may be NULL, not all.
 * guided_output_forward, preds [2 batch grid_rows, width]: o_c = c_skip z + c_out preds[r], o_u = c_skip z + c_out preds[batch
 * grid_rows + r], out = o_u + gamma (o_c - o_u), float32 in this order.  guided_output_backward: dz = c_skip dout, dpreds[r] =
 * c_out gamma dout, dpreds[batch grid_rows + r] = c_out (1 - gamma) dout (dz or dpreds may be NULL).  batch grid_rows < 2^32.
 * Plain stores, no atomics, no host reads. */
int gw_genda_input_forward(int32_t batch, int64_t grid_rows, int32_t copies, int32_t drop, int32_t w_z, int32_t w_x, int32_t w_s,
                           float sigma_data, const float* sigma, const float* z, int32_t ld_z, const float* x, int32_t ld_x, const float* c0,
                           int32_t ld_c0, const float* c1, int32_t ld_c1, const float* stat, int32_t ld_stat, float* out, int32_t ld_out,
                           float* c_noise, void* stream);
int gw_genda_input_backward(int32_t batch, int64_t grid_rows, int32_t copies, int32_t drop, int32_t w_z, int32_t w_x, int32_t n_cond,
                            float sigma_data, const float* sigma, const float* dout, int32_t ld_dout, float* dz, int32_t ld_dz, float* dx,
                            int32_t ld_dx, float* dc0, int32_t ld_dc0, float* dc1, int32_t ld_dc1, void* stream);
int gw_genda_guided_output_forward(int32_t batch, int64_t grid_rows, int32_t width, float sigma_data, float gamma, const float* sigma,
                                   const float* z, int32_t ld_z, const float* preds, int32_t ld_preds, float* out, int32_t ld_out,
                                   void* stream);
int gw_genda_guided_output_backward(int32_t batch, int64_t grid_rows, int32_t width, float sigma_data, float gamma, const float* sigma,
                                    const float* dout, int32_t ld_dout, float* dz, int32_t ld_dz, float* dpreds, int32_t ld_dpreds,
                                    void* stream);

/* =====================================================================================================================
 * GenCast's sparse processor (graph_weather/models/gencast/layers/experimental), csrc/gw_sparse_attn.hip: multi-head attention
 * masked to a sparse [n_rows, n_cols] matrix, no edge term, no head mean.  fp32, plain stores, no atomics, every sum in one fixed
 * order (bitwise reproducible), no host synchronisation; 0 rows or 0 entries: GW_OK without a launch (the caller zero-fills).
 *
 * The mask is a row-sorted CSR: the entries [row_ptr[i], row_ptr[i + 1]) belong to attending row i, entry t attends column col[t];
 * every entry is its own term (a duplicate counts twice).  Rows are in the head-major layout: head h of `heads` is the contiguous
 * segment [h dim_head, (h + 1) dim_head) of a row; heads * dim_head <= 4096 (GW_E_UNSUPPORTED above).  Per head
 *   s_t = (scale q[i, h]) . k[col[t], h],  p = softmax of s over the entries of row i,  out[i, h] = sum_t p_t v[col[t], h];
 * a row without entries gets 0.  q, out [batch n_rows, heads dim_head] and k, v [batch n_cols, heads dim_head], each with its own
 * leading dimension (column blocks of one stacked projection are read in place): `batch` >= 1 copies of the mask share the plan,
 * copy b's rows start at b n_rows resp. b n_cols (64-bit offsets).  lse [2, batch n_rows heads]: plane 0 the maximum of the scores
 * of (row, head), plane 1 log sum_t exp(s_t - max); both 0 for a row without entries.  One wave per (copy, row) covers all heads
 * with an online softmax: nothing of size n_edges x heads x dim_head or n_edges x heads is written.  Register path (16-byte loads,
 * a 64 / heads lane group per head): heads divides 64, dim_head a multiple of 4, heads * dim_head <= 2048, every leading dimension a
 * multiple of 4 and 16-byte aligned tables; anything else runs a general path (one wave per row, the heads in order).
 *
 * gw_sparse_attention_backward recomputes the probabilities from q, k and lse.  out: the forward's rows; dout like out.  One launch
 * over rows writes delta [batch n_rows heads] (scratch the caller provides) and dq (the gradient of the UNSCALED q); one launch over
 * columns walks col_pos / col_ptr (row-sorted positions grouped by column; row[t] = row of sorted entry t) and writes dk and dv.
 * Every row of dq, dk, dv is written once. */
int gw_sparse_attention_forward(int32_t batch, int32_t n_rows, int32_t n_cols, int32_t n_edges, int32_t heads, int32_t dim_head,
                                float scale, const int32_t* row_ptr, const int32_t* col, const float* q, int32_t ld_q, const float* k,
                                int32_t ld_k, const float* v, int32_t ld_v, float* out, int32_t ld_out, float* lse, void* stream);
int gw_sparse_attention_backward(int32_t batch, int32_t n_rows, int32_t n_cols, int32_t n_edges, int32_t heads, int32_t dim_head,
                                 float scale, const int32_t* row_ptr, const int32_t* col, const int32_t* row, const int32_t* col_pos,
                                 const int32_t* col_ptr, const float* q, int32_t ld_q, const float* k, int32_t ld_k, const float* v,
                                 int32_t ld_v, const float* out, int32_t ld_out, const float* dout, int32_t ld_dout, const float* lse,
                                 float* delta, float* dq, int32_t ld_dq, float* dk, int32_t ld_dk, float* dv, int32_t ld_dv,
                                 void* stream);

/* =====================================================================================================================
 * WeatherMesh's processor (graph_weather/models/weathermesh/processor.py), csrc/gw_na3d.hip: 3-D neighbourhood attention as
 * NATTEN's NeighborhoodAttention3D documents it (restated, not pinned against NATTEN): non-causal, stride 1, dilation 1, no
 * position bias.  fp32, plain stores, no atomics, every sum in one fixed order (bitwise reproducible), no host synchronisation;
 * batch 0: GW_OK without a launch.
 *
 * Tokens are the rows of a [batch, depth, height, width] volume in that order, heads * dim_head floats per row, head h the
 * contiguous segment [h dim_head, (h + 1) dim_head).  Per axis of length L with kernel k (odd, 1 <= k <= L, GW_E_BADARG else)
 * the query at index i attends to the k indices from clamp(i - k / 2, 0, L - k): windows shift inward at a border and keep k
 * keys.  Per head s = scale q . k over the kd kh kw keys of the product of the three ranges, p = softmax(s), out = sum p v.
 * q, k, v, out each have their own leading dimension (column blocks of one stacked projection are read in place); volume offsets
 * are 64-bit, batch depth height width heads < 2^31.  lse [2, rows heads]: plane 0 the maximum of the scores of (row, head),
 * plane 1 log sum exp(s - max).  dim_head <= 256 (GW_E_UNSUPPORTED above).
 *
 * Tiled path (dim_head a multiple of 4 and <= 64, kh and kw <= 7, leading dimensions multiples of 4, 16-byte aligned tables, the
 * staged planes within 160 KB of LDS): a workgroup owns 8 x 8 queries of one depth plane and one head and stages the union of
 * their windows once per key plane; the softmax is online across window rows and planes.  Anything else runs a general path (one
 * wave per token, the heads in order, everything streamed).
 *
 * gw_na3d_backward recomputes the probabilities from q, k and lse.  out: the forward's rows; dout like out.  A query-side launch
 * writes delta [rows heads] (scratch the caller provides) and dq (the gradient of the UNSCALED q); a key-side launch walks, per
 * key, the box of queries that attend to it and writes dk and dv.  Every row of dq, dk, dv is written once. */
int gw_na3d_forward(int32_t batch, int32_t depth, int32_t height, int32_t width, int32_t heads, int32_t dim_head, int32_t kd, int32_t kh,
                    int32_t kw, float scale, const float* q, int32_t ld_q, const float* k, int32_t ld_k, const float* v, int32_t ld_v,
                    float* out, int32_t ld_out, float* lse, void* stream);
int gw_na3d_backward(int32_t batch, int32_t depth, int32_t height, int32_t width, int32_t heads, int32_t dim_head, int32_t kd, int32_t kh,
                     int32_t kw, float scale, const float* q, int32_t ld_q, const float* k, int32_t ld_k, const float* v, int32_t ld_v,
                     const float* out, int32_t ld_out, const float* dout, int32_t ld_dout, const float* lse, float* delta, float* dq,
                     int32_t ld_dq, float* dk, int32_t ld_dk, float* dv, int32_t ld_dv, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GW_AMD_H */
