/* libvq_amd — C ABI of the MI355X (gfx950) frame-embedding + exact cosine k-NN path.
 *
 * The reference (adhney/video-quierer) has no FFI boundary: its boundary for this
 * path is two Python classes,
 *   FeatureExtractor        reference src/core/feature_extractor.py:21-258
 *   HNSWIndex / OptimizedHNSWIndex   reference src/indexes/hnsw.py:19-528
 * constructed at reference src/video_search_system.py:65-69 and :79-89.  The
 * build's same-named Python classes (video-quierer_amd/core/feature_extractor.py,
 * video-quierer_amd/indexes/hnsw.py) bind exactly the entry points below with
 * ctypes; INTEGRATION.md shows the binding.  Each group names the reference
 * method(s) it replaces.
 *
 * Conventions
 *   - every function returns 0 on success or a negative code; the message is in
 *     vq_last_error() (thread-local).  Wrappers raise (reference convention:
 *     log + raise, feature_extractor.py:175-177, hnsw.py:353-354).
 *   - the caller owns every host buffer (C-contiguous); the library owns device
 *     memory behind the opaque handles; *_destroy frees it.
 *   - handles are safe to share between threads (one mutex + one HIP stream per
 *     handle); ctypes releases the GIL during calls.
 *   - "_device" variants take device pointers (e.g. torch.Tensor.data_ptr()) and
 *     are asynchronous on the handle's stream until *_synchronize.
 *   - no torch / STL types cross this boundary.
 */
#ifndef VQ_AMD_H
#define VQ_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQ_OK 0
#define VQ_ERR_INVALID (-1)
#define VQ_ERR_HIP (-2)
#define VQ_ERR_STATE (-3)
#define VQ_ERR_OOM (-4)

/* ---- library ------------------------------------------------------------- */
/* Binds the calling process to one GPU (reference: device pick in
 * FeatureExtractor.__init__, feature_extractor.py:41-44).  Fails when no gfx950
 * device is visible: there is no CPU fallback. */
int vq_init(int device_ordinal);
int vq_device_count(int* count);
const char* vq_last_error(void);
const char* vq_version(void);

/* ---- encoder: FeatureExtractor._load_model / extract_batch ----------------- */
typedef struct vq_encoder vq_encoder;

typedef struct vq_vit_config {
    int32_t image_size;   /* 224 */
    int32_t patch_size;   /* 32  */
    int32_t hidden;       /* 768 */
    int32_t mlp;          /* 3072 */
    int32_t layers;       /* 12 */
    int32_t heads;        /* 12 */
    int32_t proj_dim;     /* 512 */
    float ln_eps;         /* 1e-5 */
} vq_vit_config;

/* weights: n_weights host fp32 tensors in the order of
 * video-quierer_amd/weights.py:weight_shapes() (HF state_dict names; 5 + 16*layers + 3).
 * Replaces CLIPModel.from_pretrained + .to(device) (feature_extractor.py:76-81).
 * max_batch: frames per device pass (workspace is sized for it). */
int vq_encoder_create(const vq_vit_config* cfg, const float* const* weights, int n_weights,
                      int max_batch, vq_encoder** out);
/* Same with flags: VQ_ENC_FP16 = fp16 instead of bf16 GEMM operands in every group (same MFMA rate, ~8x smaller
 * rounding error; what the Python host passes by default and the type ViT-L/14@336 is specified with; the patch
 * weights W/(255 std) are scaled by a power of two out of fp16's subnormal range and the scale is undone, exactly,
 * in the GEMM epilogue).  $VQ_AMD_DTYPE=fp16|bf16 overrides. */
#define VQ_ENC_FP16 1
/* Operand type per GEMM group (set = fp16, clear = bf16; fp32 accumulation and the same MFMA rate either way):
 * PATCH = pixels x W_patch, QKV = LN1 output x W_qkv, ATTN = q|k|v, softmax P, attention output x W_out,
 * FC1 = LN2 output x W_fc1, FC2 = quick-GELU output x W_fc2.  VQ_ENC_MIXED (all but the patch GEMM) was round 2's
 * default (which roundings the 1e-3 score tolerance can afford).  $VQ_AMD_DTYPE =
 * bf16 | fp16 | mixed | mask:<bits 0-4> overrides the flags. */
#define VQ_ENC_F16_PATCH 0x100
#define VQ_ENC_F16_QKV 0x200
#define VQ_ENC_F16_ATTN 0x400
#define VQ_ENC_F16_FC1 0x800
#define VQ_ENC_F16_FC2 0x1000
#define VQ_ENC_MIXED (VQ_ENC_F16_QKV | VQ_ENC_F16_ATTN | VQ_ENC_F16_FC1 | VQ_ENC_F16_FC2)
/* VQ_ENC_CONCURRENT: the caller keeps several encoder handles busy at once on separate HIP streams.  The
 * N = hidden GEMMs then keep 256-row tiles (150 dense workgroups at batch 256, leaving CUs to the other
 * streams: +7 % aggregate frames/s measured with 3 streams) instead of the 160-row tiles that spread one
 * pass over 240 CUs (+5 % for a single stream). */
#define VQ_ENC_CONCURRENT 2
int vq_encoder_create_ex(const vq_vit_config* cfg, const float* const* weights, int n_weights,
                         int max_batch, int flags, vq_encoder** out);
/* Another handle on the SAME device weights (own stream, workspace and profiling state): for callers that keep
 * several batches in flight.  flags: VQ_ENC_CONCURRENT only (operand types are the parent's).  The weights live
 * until the last handle using them is destroyed, in any order. */
int vq_encoder_create_shared(vq_encoder* parent, int max_batch, int flags, vq_encoder** out);
int vq_encoder_destroy(vq_encoder* enc);

/* extract_batch (feature_extractor.py:137-177) for uint8 frames already at
 * image_size x image_size: frames [n][S][S][3] -> out [n][proj_dim] fp32,
 * L2-normalised.  swap_rb=1 is the ndarray path (BGR->RGB, :111-112), 0 the PIL
 * path.  Any n >= 0 (processed in max_batch slices); synchronous. */
int vq_encoder_encode_u8(vq_encoder* enc, const uint8_t* frames, int n, int swap_rb, float* out);

/* Same, device-resident input/output, n <= max_batch, asynchronous.
 * d_out_f16 (optional, may be NULL) receives an fp16 copy of the embeddings. */
int vq_encoder_encode_u8_device(vq_encoder* enc, const void* d_frames, int n, int swap_rb,
                                void* d_out_f32, void* d_out_f16);
/* Pinned host staging: two slots of max_batch frames each.  The host side assembles frames straight
 * into a slot (one copy instead of two) and encodes from it; while slot s is being encoded (the call
 * blocks only its own thread) another thread may fill slot 1-s.  n <= max_batch. */
int vq_encoder_staging(vq_encoder* enc, int slot, uint8_t** host_ptr, size_t* bytes);
int vq_encoder_encode_staged(vq_encoder* enc, int slot, int n, int swap_rb, float* out);
/* Pipelined ingest of host frames (what extract_from_video_frames, feature_extractor.py:179-209, loops over):
 *   vq_encoder_stage_frames   gathers n separately allocated S x S x 3 uint8 frames (a Python list of ndarray
 *                             frames) into pinned slot 0/1 on up to n_threads host threads;
 *   vq_encoder_submit_staged  enqueues upload (copy stream) -> forward -> download for that slot and returns;
 *   vq_encoder_wait_staged    blocks until the slot's batch is done and copies out [n][proj_dim] fp32.
 * With two slots the upload and the host gather of batch i+1 overlap the forward pass of batch i. */
int vq_encoder_stage_frames(vq_encoder* enc, int slot, const uint8_t* const* frames, int n, int n_threads);
int vq_encoder_submit_staged(vq_encoder* enc, int slot, int n, int swap_rb);
int vq_encoder_wait_staged(vq_encoder* enc, int slot, float* out);
int vq_encoder_synchronize(vq_encoder* enc);
/* Run this handle's kernels on a caller-owned HIP stream (e.g. torch's current
 * stream, so RCCL collectives issued by torch order after the encode without a
 * host sync).  NULL restores the handle's own stream. */
int vq_encoder_set_stream(vq_encoder* enc, void* hip_stream);
int vq_encoder_output_dim(vq_encoder* enc, int* dim);

/* Per-kernel-class device timing with HIP events on the encoder's stream
 * (bench.py roofline leg).  Between begin/end every launch is bracketed by
 * events; end() reports total ms and launch count per class. */
#define VQ_ENC_NCLASS 11
int vq_encoder_profile_begin(vq_encoder* enc);
int vq_encoder_profile_end(vq_encoder* enc, float* ms /*[VQ_ENC_NCLASS]*/, int* launches /*[VQ_ENC_NCLASS]*/);
const char* vq_encoder_profile_class_name(int cls);
/* Median elapsed time of an EMPTY event bracket on the encoder's stream: what a bracket adds to the kernel it holds. */
int vq_encoder_profile_bracket_overhead(vq_encoder* enc, float* ms);

/* Test hooks: run only the first `layers` transformer blocks (<0: all), and copy
 * an internal activation to the host as fp32: "x" [n*T][hidden] residual stream,
 * "h" LN output, "qkv", "att", "mlp" (bf16 widened); "xl" [n*T][hidden]: the low half of the split residual
 * stream as its raw bytes 0..255 (fp8 e4m3 of (x - xh) * 512; the reader decodes).
 * vq_encoder_debug_keep_stream(on): a layer-limited pass runs its blocks exactly as the full pass runs them
 * (the split 16 + 8-bit stream and the epilogue modes follow the model's depth and the CLS-only last block,
 * not the limit) and leaves x, xh, xl as they are at that point; its pooled output is meaningless.  Off
 * (the default): layer-limited passes keep the fp32 stream.  vq_encoder_debug_stream_is_split: whether the
 * last pass left the stream as the pair xh + xl (1) or as the fp32 x (0). */
int vq_encoder_debug_set_layers(vq_encoder* enc, int layers);
int vq_encoder_debug_keep_stream(vq_encoder* enc, int on);
int vq_encoder_debug_stream_is_split(vq_encoder* enc, int* split);
int vq_encoder_debug_read(vq_encoder* enc, const char* name, int rows, float* out);

/* C[M][N] = A[M][K] * W[N][K]^T through the production MFMA mainloops (inputs
 * rounded from the given fp32, fp32 accumulate) — unit-test hook.
 * flags: bit 0 = fp16 inputs (else bf16); bits 1-5 = kernel (the GemmKernel ids of
 * csrc/gemm_dispatch.h: 0 auto, 1 = 128x128 two-phase, 2 = 256x256 phased, ...). */
int vq_debug_gemm(const float* A, const float* W, int M, int N, int K, int flags, float* C);

/* What the GEMM dispatch (csrc/gemm_dispatch.h) would launch for C[M][N] with leading dimensions lda / ldw in this
 * build and with this process's environment switches: n_steps (1 or 2) launches of `kernel` (a GemmKernel id) on
 * `rows` rows from row `row0`, `tiles_per_wg` tiles per workgroup.  row_in: the epilogue consumes LayerNorm row
 * statistics (q|k|v, fc1).  force: the kernel id of $VQ_AMD_GEMM.  Pure host arithmetic: needs neither vq_init nor
 * a device.  An id that this build does not carry returns VQ_ERR_INVALID. */
int vq_debug_gemm_plan(int M, int N, int K, int lda, int ldw, int row_in, int force, int* n_steps,
                       int* kernel /*[2]*/, int* rows /*[2]*/, int* row0 /*[2]*/, int* tiles_per_wg /*[2]*/);

/* ---- text tower: FeatureExtractor.extract_text_features (feature_extractor.py:218-234) ------------ */
/* CLIPTextModel + text_projection on token ids (the tokenizer stays on the host).  weights: host fp32
 * tensors in the order of video-quierer_amd/weights.py:text_weight_shapes() (2 + 16*layers + 3).
 * flags as vq_encoder_create_ex. */
typedef struct vq_encoder vq_text_encoder;
typedef struct vq_text_config {
    int32_t vocab;          /* 49408 */
    int32_t max_positions;  /* 77 */
    int32_t hidden;         /* 512 */
    int32_t mlp;            /* 2048 */
    int32_t layers;         /* 12 */
    int32_t heads;          /* 8 */
    int32_t proj_dim;       /* 512 */
    int32_t eos_token_id;   /* 49407 */
    float ln_eps;           /* 1e-5 */
} vq_text_config;
int vq_text_encoder_create(const vq_text_config* cfg, const float* const* weights, int n_weights,
                           int max_batch, int flags, vq_text_encoder** out);
/* ids [n][seq_len] (seq_len <= max_positions; every row holds an eos token, as the tokenizer produces):
 * out [n][proj_dim] fp32, L2-normalised.  Rows are padded to max_positions with eos internally (the
 * causal mask makes the padding invisible to the pooled EOS position).  Synchronous; any n. */
int vq_text_encoder_encode_ids(vq_text_encoder* enc, const int32_t* ids, int n, int seq_len, float* out);
int vq_text_encoder_destroy(vq_text_encoder* enc);

/* What a forward pass of n inputs would launch, and where a handle's buffers would lie (csrc/encoder_plan.h), for a
 * handle that is never made: one of `vit` / `text` (the other NULL), max_batch, the create flags, `shared` (the handle
 * of vq_encoder_create_shared: workspace only), the two debug switches, this process's environment.  Row counts of the
 * GEMMs (qkv and fc1 / out_proj / fc2 / patch embedding / the CLS-only block), the kernel id each hands to the GEMM
 * dispatch, the patchify kernel (0 none, 1 8-pixel, 2 generic) and the attention kernel (0 causal workgroup, 1 T = 50
 * tile, 2 T <= 64 tile, 3 per-wave stream, 4 32-row workgroup, 5 64-row workgroup), the residual stream's form, and
 * byte offsets from the arena's base.  resid_modes (optional) [2 * layers]: the mode bits (1 reads xh + xl, 2 writes
 * xl, 4 writes the fp32 x) of each block's out_proj and fc2 epilogue, -1 where the pass runs neither on every row.
 * Pure host arithmetic: needs neither vq_init nor a device. */
typedef struct vq_encoder_plan {
    int64_t rows, rows_gemm, rows_out, rows_fc2, prows, prows_gemm, rows_cls;
    int64_t k_patch, k_qkv, k_out, k_fc1, k_fc2, k_cls;
    int64_t patchify, attention, layers_run, cls_only_last, fc2_splits, split, stream_left_split;
    int64_t rows_pad, prow_pad, arena_bytes, workspace_end;      /* workspace_end: where mlp, the last buffer, ends */
    int64_t off_input, off_rowidx, off_ps, off_x, off_out, off_h, off_xl, off_qkv, off_att, off_mlp;   /* input: frames or ids; rowidx: -1 for images */
} vq_encoder_plan;
int vq_debug_encoder_plan(const vq_vit_config* vit, const vq_text_config* text, int max_batch, int n, int flags, int shared,
                          int run_layers, int keep_stream, vq_encoder_plan* out, int* resid_modes);

/* Mainloop stamps / ablations / clock probes are not product entry points: include/vq_amd_diag.h (`make DIAG=1`). */

/* ---- index: HNSWIndex.add / search / size / save / load --------------------- */
typedef struct vq_index vq_index;

/* HNSWIndex.__init__ (hnsw.py:25-57).  The graph parameters (M, ef_*) have no
 * device-side meaning: the index is an exact scan. */
int vq_index_create(int dim, vq_index** out);
int vq_index_destroy(vq_index* idx);

/* add / add_batch (hnsw.py:150-236): appends n rows.  normalize=1 divides each
 * row by its L2 norm on the device (fixed-order fp64 chain, see oracle/knn_oracle.c);
 * normalize=0 stores the rows as given (the Python wrapper normalises with numpy
 * exactly like the reference, hnsw.py:157, and passes 0).  Rows stored as given are MEASURED, not trusted:
 * the index keeps the range of |row|^2 it holds; while 0.5 <= |row|^2 <= 2 the fp16 scan stays available
 * with its error bound scaled by the largest |row|, outside that range mode 0 uses the exact scan and
 * mode 2 is refused. */
int vq_index_add(vq_index* idx, const float* rows, int64_t n, int normalize);
int vq_index_add_device(vq_index* idx, const void* d_rows_f32, int64_t n, int normalize);
/* Re-add of an id the index already holds (hnsw.py:160 `self.data[node_id] = vector`: a dict assignment): replaces
 * stored rows IN PLACE — fp32 master, fp16 scan copy and the |row|^2 range — without touching the other rows.
 * rows [n][dim] (host), row_numbers [n] in [0, size).  A row named more than once keeps its LAST update, as the
 * reference's sequential assignments do.  normalize as vq_index_add.  The result is bit-identical to an index built
 * from scratch with the updated rows.  Synchronous. */
int vq_index_update_rows(vq_index* idx, const float* rows, const int64_t* row_numbers, int64_t n, int normalize);
/* Removal of rows (the reference drops a video's frames from its index, video_search_system.py:427-463): row_numbers [n], each in
 * [0, size), else VQ_ERR_INVALID and the index is unchanged; a row named twice is removed once; n = 0 is a no-op.  The survivors
 * keep their relative order and are renumbered densely (row r becomes r minus the removed rows below it), and the stored rows
 * (fp32 master and fp16 scan copy) are bit-identical to what vq_index_add of the survivors stores.  Id ranks that cover the index
 * stay valid: a survivor's new rank is its old rank minus the removed rows of smaller rank — exactly the ranks of the surviving ids
 * — so no vq_index_set_id_ranks call is needed; stale ranks are dropped.  Group labels that cover the index stay valid too, with a
 * canonical new numbering: groups left without rows are dropped and the others keep their old order, renumbered densely (old
 * group g becomes g minus the emptied groups below it); the result is what vq_index_set_groups would build from those labels.
 * Stale labels are dropped.  The |row|^2 range is kept (it still covers every survivor).  Rows move on the device, through at
 * most 256 MiB of scratch.  Synchronous.  A sharded index (vq_index_search_sharded) is not renumbered across shards: removing
 * rows from one shard shifts the row_offset of every shard behind it, which the caller passes. */
int vq_index_remove_rows(vq_index* idx, const int64_t* row_numbers, int64_t n);
int vq_index_size(vq_index* idx, int64_t* n);
int vq_index_clear(vq_index* idx);
/* The tie order of the result lists.  The reference returns `sorted(candidates)[:k]` over (distance, id) tuples
 * (hnsw.py:269, :518): rows at EQUAL distance (duplicate frames) come back in the order of the caller's ids — strings
 * f"{video_id}_{i}" under video_search_system.py:164-166, where "video0_10" sorts before "video0_2".  The library sees row
 * numbers only, so the host hands it rank_of_row[r] = position of row r's id in the caller's id order (a permutation of
 * 0..n-1, n = the current size; checked).  Every search then selects and orders by (dist, rank) on the device and still
 * reports ROW numbers.  n = 0 (rank_of_row may be NULL) returns to (dist, row) order.  Ranks describe the rows present when
 * they were set: after vq_index_add* a search is refused (VQ_ERR_INVALID) until the ranks are set again or cleared;
 * vq_index_update_rows keeps them (same ids), vq_index_clear drops them.  Synchronous.  vq_index_search_sharded orders
 * ties ACROSS shards by global row number whatever the shards' ranks say. */
int vq_index_set_id_ranks(vq_index* idx, const int32_t* rank_of_row, int64_t n);

/* search / search_batch (hnsw.py:238-300, 488-528) as an exact scan:
 *   dist = fp32(1 - fp32(dot(row, q))), k smallest, ordered by (dist, row) — or (dist, id rank) once
 *   vq_index_set_id_ranks has been called.
 * queries [nq][dim] are used as given (the wrapper does query / ||query|| with numpy, hnsw.py:250).  The
 * fp16 path's exactness bound scales with each query's own norm while 0.25 <= |q|^2 <= 4; a query outside that
 * range (or not finite) is outside what fp16 operands can bound and is answered by the exact scan instead
 * (device-side fallback), so un-normalised queries stay exact at any scale.  ids/dist are [nq][k]; unused slots
 * (k > size) are id -1 / dist +inf.  mode: 0 auto (fp16 scan from 16,384 rows and k <= 100: the API takes k up to 50, src/api/routes.py:58, and the caller searches for k * 2, video_search_system.py:297), 1 exact
 * fp32-master scan, 2 fp16 MFMA scan + exact re-score with proof (unproven queries are redone by the
 * exact scan, on the device: nothing is read back).  vq_index_search_device is asynchronous on the index's
 * stream in every mode, with one exception: the first search after a vq_index_add_device(normalize=0) waits
 * for the stream once to read the |row|^2 range those rows were measured at (the host-side adds read it
 * before they return).  vq_index_last_search_stats waits for that stream. */
int vq_index_search(vq_index* idx, const float* queries, int nq, int k, int mode,
                    int32_t* ids, float* dist);
int vq_index_search_device(vq_index* idx, const void* d_queries_f32, int nq, int k, int mode,
                           void* d_ids_i32, void* d_dist_f32);
int vq_index_synchronize(vq_index* idx);
int vq_index_set_stream(vq_index* idx, void* hip_stream);

/* Grouped search: the k best GROUPS (videos), one best row (frame) each — what video_search_system.py:296-342 builds on the
 * host by over-fetching search(q, k * 2) and keeping each video's first row, which returns fewer than k videos once the top
 * 2k frames span fewer than k of them.
 *   vq_index_set_groups: group_of_row [n] labels every row, dense in [0, n_groups) (every group holds a row), n = the current
 *   size; all of it is checked (VQ_ERR_INVALID).  n = 0 clears the labels.  The library keeps them with a by-group row list.
 *   Lifetime as the id ranks: after vq_index_add* a grouped search is refused (VQ_ERR_INVALID) until the labels are set again;
 *   vq_index_update_rows keeps them, vq_index_clear drops them.  Synchronous.
 *   vq_index_search_grouped: per query, a group's best row is its row with the smallest (distance, tie rank) — distance and
 *   tie rank as vq_index_search — and groups are ordered by their best row's (distance, tie rank).  groups / rows / dist are
 *   [nq][k]: the first min(k, n_groups) groups, their best row numbers and distances; unused slots are -1 / -1 / +inf.  This is
 *   the plain search's exhaustive (distance, id) list with every row dropped whose group came earlier.  mode as vq_index_search
 *   (2 = fp16 group-max scan + exact re-score of the candidate groups with proof, for dim 256, 512 or 768; mode 0 takes it
 *   under the plain search's rule); queries the proof does not cover (|q|^2 outside [0.25, 4], not finite, too many candidate
 *   groups) are answered by the exact path on the device.  The _device form takes device pointers and is asynchronous on the
 *   index's stream.  After a grouped search vq_index_last_search_stats reports [0] queries answered by the fp16 path, [1] rows
 *   re-scored exactly (summed over queries), [2] queries answered by the exact path. */
int vq_index_set_groups(vq_index* idx, const int32_t* group_of_row, int64_t n, int32_t n_groups);
int vq_index_search_grouped(vq_index* idx, const float* queries, int nq, int k, int mode,
                            int32_t* groups, int32_t* rows, float* dist);
int vq_index_search_grouped_device(vq_index* idx, const void* d_queries_f32, int nq, int k, int mode,
                                   void* d_groups_i32, void* d_rows_i32, void* d_dist_f32);

/* Filtered search: the plain or grouped search restricted to the rows S whose group label (vq_index_set_groups) is in the set
 * groups [n_sel] (exclude = 0) or not in it (exclude = 1) — "within this video", "more like this from other videos", "within
 * this collection".  One filter applies to every query of the call.
 *   groups is host memory in every form (it is small, and the host sizes S from its own copy of the group offsets, which
 *   vq_index_set_groups and vq_index_remove_rows keep).  Duplicates are allowed; a label outside [0, n_groups) is
 *   VQ_ERR_INVALID.  The labels' lifetime is the grouped search's: stale or missing labels are refused (VQ_ERR_INVALID).
 *   vq_index_search_filtered returns what vq_index_search would return on an index holding only the rows of S, in their
 *   order, with the same tie ranks restricted to S: the same distances and the same (distance, tie rank) order bit for bit,
 *   rows reported as row numbers of the full index, unused slots (k > |S|) -1 / +inf.
 *   vq_index_search_grouped_filtered returns what vq_index_search_grouped would return on that index: the first
 *   min(k, allowed groups) groups, labels of the full index.
 *   n_sel = 0, exclude = 0: every slot empty.  n_sel = 0, exclude = 1: exactly vq_index_search / vq_index_search_grouped.
 *   mode: 1 = the exact gather path (any nq, k <= 1024, any dim: S's row list from the by-group row list, the listed rows'
 *   fp64-chain distances, the exact path's selection).  2 = the masked fp16 scan (a disallowed video's streams are not read,
 *   disallowed rows of mixed streams never score) with an exact re-score under the unfiltered proof, every floor taken over
 *   allowed rows; queries it does not prove are redone by a masked exact fallback on the device.  It exists for dim 256, 512
 *   or 768, nq <= 96, k <= 100 and near-unit rows; elsewhere mode 2 is VQ_ERR_INVALID, refused before any work is queued.
 *   0 = the library chooses: the fp16 scan where it exists, on 16,384 rows or more, once S holds at least half the rows (a
 *   fifth for more than 4 queries; measured crossover), else the gather path.  An empty exclude list runs the unfiltered
 *   search in any mode.  The _device forms take device queries and results and are asynchronous on the index's stream (the
 *   filter list goes up from a ring of four pinned slots: a call waits only for the list copy of the call four before it).
 *   vq_index_last_search_stats after a filtered search: [0] queries proven on the fp16 path (directly or after rescans), [1]
 *   queries that needed rescans, [2] queries answered exactly (gather path or fallback); after a grouped filtered search the
 *   grouped meanings hold. */
int vq_index_search_filtered(vq_index* idx, const float* queries, int nq, int k, int mode,
                             const int32_t* groups, int32_t n_sel, int exclude, int32_t* ids, float* dist);
int vq_index_search_filtered_device(vq_index* idx, const void* d_queries_f32, int nq, int k, int mode,
                                    const int32_t* groups, int32_t n_sel, int exclude, void* d_ids_i32, void* d_dist_f32);
int vq_index_search_grouped_filtered(vq_index* idx, const float* queries, int nq, int k, int mode,
                                     const int32_t* groups, int32_t n_sel, int exclude,
                                     int32_t* groups_out, int32_t* rows, float* dist);
int vq_index_search_grouped_filtered_device(vq_index* idx, const void* d_queries_f32, int nq, int k, int mode,
                                            const int32_t* groups, int32_t n_sel, int exclude,
                                            void* d_groups_i32, void* d_rows_i32, void* d_dist_f32);

/* Clip search: the k groups (videos) most similar to a SET of query frames q_0 .. q_{m-1} — "more like this video", "is this
 * upload a cut or a re-encode of something indexed", several example frames that should all be found.
 *   d(i, g) = the smallest distance of q_i to a row of group g (distance and tie rank as vq_index_search; the row that attains
 *   it has the smallest (distance, tie rank));  D(g) = fp32((d(0,g) + d(1,g) + ... + d(m-1,g), added in fp64 in this order) /
 *   m);  the answer is the first min(k, allowed groups) groups by (D, label) ascending, unused slots -1 / +inf.  It is
 *   one-directional: every query frame looks for its best match in the video, the video's other frames cost nothing.  For
 *   near-unit rows and queries the fp64 sum is exact, so the order of the frames does not change D.
 *   match_rows [k][m] (or NULL): the row of result group j that attains d(i, group j), full-index row numbers; -1 in unused slots.
 *   groups / n_sel / exclude: the filter of vq_index_search_filtered (host memory, duplicates allowed, a label outside
 *   [0, n_groups) is VQ_ERR_INVALID; stale or missing labels and stale id ranks are refused before any work is queued).
 *   n_sel = 0, exclude = 1 is the unfiltered call; n_sel = 0, exclude = 0 returns every slot empty.  A group's D does not
 *   depend on other groups: the filtered answer is the unfiltered ranking with the disallowed groups struck out.
 *   Limits: 1 <= m <= 4096, 1 <= k <= 1024 (else VQ_ERR_INVALID).
 *   mode: 1 = exact (the plain path's distances per query chunk, group minima, per-group fp64 sums).  2 = fp16 with proof: one
 *   pass of a 256-query MFMA tile scan per 256 query frames leaves each (frame, group) maximum, groups whose mean fp16 score is
 *   within twice the mean error bound of the k-th are re-scored exactly over all their rows; dim 256, 512 or 768 and near-unit
 *   rows, else VQ_ERR_INVALID before any work is queued.  A call it cannot prove (a query with |q|^2 outside [0.25, 4] or not
 *   finite, more than 16 Mi candidate (group, frame) pairs) is redone by the exact path on the device.  0 = the plain search's
 *   rule: fp16 where it exists, from 16,384 rows.
 *   Scratch is bounded: the frames are processed in chunks that keep the per-(frame, group) tables within 256 MiB and the exact
 *   distances within 512 MiB; the candidates' keys take at most 128 MiB; per-group arrays take 40 B per group.
 *   The _device form takes device queries and results and is asynchronous on the index's stream; nothing is read back.
 *   vq_index_last_search_stats afterwards: [0] 1 if the fp16 path proved the answer, [1] rows re-scored exactly (candidate rows
 *   x m), [2] 1 if the exact path answered. */
int vq_index_search_set(vq_index* idx, const float* queries /*[m][dim]*/, int m, int k, int mode,
                        const int32_t* groups, int32_t n_sel, int exclude,
                        int32_t* groups_out /*[k]*/, float* dist_out /*[k]*/, int32_t* match_rows /*[k][m] or NULL*/);
int vq_index_search_set_device(vq_index* idx, const void* d_queries_f32, int m, int k, int mode,
                               const int32_t* groups, int32_t n_sel, int exclude,
                               void* d_groups_i32, void* d_dist_f32, void* d_match_rows_i32 /*or NULL*/);

/* Distinct-moment search: the k best rows such that two results of the same group (video) lie at least min_gap positions
 * apart — "the three places in this lecture where the whiteboard is shown".  Between the plain search (one moment k times)
 * and the grouped search (one row per video).
 *   vq_index_set_positions: pos_of_row [n], one int32 per row of the caller's choosing (a frame ordinal, a timestamp in ms); it
 *   need not be monotone in row order and may repeat.  n = the current size; n = 0 clears the positions.  Lifetime: after
 *   vq_index_add* a distinct search is refused (VQ_ERR_INVALID) until the positions are set again; vq_index_update_rows keeps
 *   them; vq_index_clear drops them; vq_index_remove_rows DROPS them too (they are not compacted: set them again).
 *   Synchronous.
 *   vq_index_search_distinct: let L be the exhaustive list of all rows in vq_index_search's order ((dist, row), or (dist, id
 *   rank) once ranks are set).  Walk L and keep a row unless an already kept row of the SAME group (vq_index_set_groups) lies
 *   at |position difference| < min_gap (min_gap >= 0; the difference is taken in 64-bit).  ids / dist [nq][k] are the first k
 *   kept rows (row numbers) and their distances in L's order; unused slots are -1 / +inf.  min_gap = 0 is exactly
 *   vq_index_search; a min_gap above every position difference gives the rows and distances of vq_index_search_grouped.
 *   Limits: 1 <= k <= 1024, min_gap >= 0.  Stale or missing labels, positions or id ranks are refused before any work is queued.
 *   How it runs: the plain search fetches a prefix of L of depth D per query and one wave per query walks it; greedy over a
 *   prefix keeps exactly the kept rows among it, so k kept rows (or D = size) prove the answer.  Queries left short are redone
 *   exactly on the device: fp64-chain distances to all rows, a per-(query, group) greedy walk that gives +inf to every row of
 *   the group it does not keep, then the exact path's selection; sliced so that the distances stay within 512 MiB.  The
 *   launches queued depend on the shapes only.
 *   Depth rule: D = max(64, 4 k), capped by the size and by the producer's k limit (fp16 scan: 100, exact selection: 1024);
 *   D = k when min_gap = 0 or k = 1.  $VQ_AMD_DISTINCT_DEPTH (tests only, read per call) replaces the rule, under the same caps.
 *   mode is vq_index_search's and chooses only the producer of the prefix (0: the fp16 scan from 16,384 rows); the answer is
 *   bit-identical in every mode.  The _device form takes device pointers, is asynchronous on the index's stream and reads
 *   nothing back.  vq_index_last_search_stats afterwards: [0] queries proven on the prefix, [1] prefix entries walked (summed
 *   over queries), [2] queries answered by the exact path.
 *   vq_debug_distinct_plan (host only, as vq_debug_scan_plan): the depth D a call of this shape fetches, the producer (0 exact
 *   distances + selection, 1 fp16 scan) and the number of redo slices it queues. */
int vq_index_set_positions(vq_index* idx, const int32_t* pos_of_row, int64_t n);
int vq_index_search_distinct(vq_index* idx, const float* queries, int nq, int k, int mode, int64_t min_gap,
                             int32_t* ids, float* dist);
int vq_index_search_distinct_device(vq_index* idx, const void* d_queries_f32, int nq, int k, int mode, int64_t min_gap,
                                    void* d_ids_i32, void* d_dist_f32);
int vq_debug_distinct_plan(int64_t n, int nq, int k, int64_t min_gap, int mode,
                           int64_t* depth, int* producer, int* redo_slices);

/* Diverse search: the k best rows such that no two results look alike — suppression in embedding space.  A static shot, an
 * intro that sits in every episode and bit-exact re-uploads otherwise take all k slots of vq_index_search; the grouped and
 * distinct searches suppress by position only.  No labels or positions are needed; id ranks only order L.
 *   Definition (the order of operations is part of it).  L = the exhaustive list of all rows in vq_index_search's order ((dist,
 *   row), or (dist, id rank) once ranks are set).  d(a, b) = 1.0f - fp32(sum_i (double)x_a[i] * (double)x_b[i]), summed in index
 *   order: the keyframe summary's row-to-row distance, i.e. vq_index_search's distance with row b as the query; it is symmetric
 *   bit for bit.  Walk L and keep a row r unless min_dist > 0 and an already kept row s has d(r, s) < min_dist (an fp32
 *   compare, strict).  ids / dist [nq][k] are the first k kept rows (row numbers) and their distances to the query in L's
 *   order; unused slots are -1 / +inf.
 *   Consequences: min_dist = 0 is exactly vq_index_search, even with bit-exact copies in the index, whose d may be -1.2e-7 (why
 *   the rule carries min_dist > 0); a min_dist above every pair distance (3.0f) returns one row; the answer for k is a prefix
 *   of the answer for k' > k.  Rows that are not finite are outside the definition: such a call may return anything, but ends.
 *   Limits: 1 <= k <= 256, min_dist >= 0 and not NaN, nq >= 1; a violation is VQ_ERR_INVALID, judged before the device is asked
 *   for, and the message names the argument.  Stale id ranks are refused before any work is queued.  An empty index returns
 *   every slot empty.
 *   How it runs: the plain search fetches a prefix of L of depth D per query; a pair pass decides d(r_i, r_j) < min_dist for
 *   the pairs i < j of each prefix (the same fp64 chain) into a bit matrix [nq][D][ceil(D / 64)] of 64-bit words; one wave per
 *   query walks the prefix with the suppressed set across its lanes.  A row's fate depends only on rows before it in L, so k
 *   kept rows (or D = size) prove the answer.  Queries left short are redone exactly on the device in k rounds over their
 *   distances to all rows (sliced to 512 MiB): pick the live row with the smallest (dist, tie), then give +inf to every live
 *   row closer than min_dist to it (row by row while at most 4 queries of a slice are filed, by exact-distance tiles beyond).  The launches queued depend on the shapes and k only; nothing is read back in between.
 *   Depth rule: D = max(256, 8 k), capped by the size and by the producer's k limit (fp16 scan: 100, exact selection: 1024);
 *   D = k when min_dist = 0 or k = 1.  $VQ_AMD_DIVERSE_DEPTH (tests only, read per call) replaces the rule, under the same caps.
 *   mode is vq_index_search's and chooses only the producer of the prefix (0: the fp16 scan from 16,384 rows); the answer is
 *   bit-identical in every mode.  The _device form takes device pointers, is asynchronous on the index's stream and reads
 *   nothing back.  vq_index_last_search_stats afterwards: [0] queries proven on the prefix, [1] prefix entries walked (summed
 *   over queries), [2] queries answered by the redo.
 *   vq_debug_diverse_plan (host only, as vq_debug_distinct_plan): the depth D a call of this shape fetches, the producer (0
 *   exact distances + selection, 1 fp16 scan), the bytes of the bit matrix (nq * D * ceil(D / 64) * 8; 0 when no pair pass
 *   runs: min_dist = 0 or D = 1), the redo slices it queues and the kernels queued behind the plain search's own. */
int vq_index_search_diverse(vq_index* idx, const float* queries, int nq, int k, int mode, float min_dist,
                            int32_t* ids, float* dist);
int vq_index_search_diverse_device(vq_index* idx, const void* d_queries_f32, int nq, int k, int mode, float min_dist,
                                   void* d_ids_i32, void* d_dist_f32);
int vq_debug_diverse_plan(int64_t n, int nq, int k, float min_dist, int mode,
                          int64_t* depth, int* producer, int64_t* pair_bytes, int* redo_slices, int* launches);

/* Sequence search: the k groups (videos) that show a list of steps IN ORDER — a storyboard of text prompts ("opens the door,
 * then sits down, then picks up the phone"), or "where, in which video, does this clip occur".  The clip search scores every
 * step on its own, so a video that shows the steps reversed or minutes apart scores the same; this one joins the steps along
 * the position axis (vq_index_set_positions).
 *   Steps q_0 .. q_{m-1} [m][dim], used as given.  d(j, r) = the distance of q_j to row r exactly as vq_index_search reports
 *   it (fp32 of the fixed-order fp64 chain); tie(r) = the row number, or the id rank once ranks are set.
 *   A CHAIN in group g is a list of rows r_0 .. r_{m-1}, all of g, with min_gap <= pos(r_{j+1}) - pos(r_j) <= max_gap for every
 *   j (the difference taken in 64-bit; 1 <= min_gap <= max_gap, both int64).  Positions therefore increase strictly: two rows
 *   at one position never follow each other.
 *   Cost, by dynamic programme (the order of the additions is part of the definition):  C_0(r) = (double)d(0, r);  for j >= 1,
 *   C_j(r) = C_{j-1}(p*) + (double)d(j, r) added in fp64, where p* is the admissible predecessor of r (same group, position
 *   difference within the gaps, C_{j-1} defined) with the smallest (C_{j-1}(p), tie(p));  C_j(r) is undefined when there is none.
 *   A group's result: the row e with the smallest (C_{m-1}(e), tie(e));  D(g) = fp32(C_{m-1}(e) / m);  its chain is e followed
 *   back through the p*.  A group with no defined C_{m-1} has no result and never appears.
 *   The answer is the first min(k, allowed groups that hold a chain) groups by (D, label) ascending; chain_rows [k][m] (or
 *   NULL): full-index row numbers in step order; unused slots are -1 / +inf / -1.
 *   Limits: 1 <= m <= 64, 1 <= k <= 1024, 1 <= min_gap <= max_gap (else VQ_ERR_INVALID).
 *   groups / n_sel / exclude: the filter of vq_index_search_filtered in host memory, with the checks and the two empty-list
 *   cases of vq_index_search_set (n_sel = 0, exclude = 1: unfiltered; n_sel = 0, exclude = 0: every slot empty).  A group's D
 *   does not depend on other groups.  Stale or missing labels, positions or id ranks are refused before any work is queued.
 *   Consequences: m = 1 gives the groups, rows and distances of vq_index_search_grouped (filtered: _grouped_filtered);
 *   D_seq(g) >= D_set(g) of vq_index_search_set in mode 1 for every group returned.
 *   How it runs (csrc/knn_sequence.h): exact only, no mode.  Per chunk of steps the plain search's exact distances [chunk][n]
 *   (chunks keep them within 512 MiB), then one workgroup per allowed group runs the chunk's steps over the group's rows in
 *   (position, tie) order — a second permutation next to the by-group row list, sorted on the host and uploaded by the first
 *   sequence search after the labels, the positions or the id ranks changed (that one call waits for the stream once).  A row's
 *   admissible predecessors are a contiguous range of that order, found once per row and launch; the range minimum of the
 *   (64-bit order-preserving cost key, tie) reads at most 126 + L / 64 entries per row and step in a group of L rows.  Groups
 *   of at most 4,096 rows keep positions, ties, ranges and two cost arrays in LDS (36 B per row); longer groups run the same
 *   arithmetic over global arrays with one more level of minima (at most 252 + L / 4096 reads; one group of a million rows is
 *   legal: a bound, not a target).  The fp64 costs [n] are
 *   carried between chunks.  A small kernel turns C_{m-1} into each group's (D, label) key and end row; the clip search's
 *   selection takes the k smallest.  Chains: the DP kernels write a back-pointer table [m-1][n] int32 when that stays within
 *   256 MiB; otherwise one workgroup per winner runs its group's DP again and keeps the back-pointers of one slice of steps at a
 *   time, last slice first (slice [s][n] int32 <= 256 MiB, s >= 1: above 2^26 rows it is 4 B per row).
 *   Scratch beyond that: 24 B per row of cost keys, 12 B per row of ranges and block minima, 12 B per row for the order itself,
 *   and the clip search's per-group selection arrays.  The launches queued depend on the shapes only.
 *   The _device form takes device steps and results, is asynchronous on the index's stream and reads nothing back.
 *   vq_index_last_search_stats afterwards: [0] the groups that hold a chain, [1] the allowed groups run by the global form,
 *   [2] the step chunks.
 *   $VQ_AMD_SEQ_LDS_ROWS (the LDS form's row limit, at most 4,096), $VQ_AMD_SEQ_DIST_BYTES (the distance budget) and
 *   $VQ_AMD_SEQ_BP_BYTES (the back-pointer budget): tests only, read per call.
 *   vq_debug_sequence_plan (host only, as vq_debug_distinct_plan): for n rows whose longest group holds largest_group rows — the
 *   step chunks, the LDS form's row limit and its dynamic LDS bytes, groups_global_form = 1 when the longest group (so at least
 *   one) takes the global form, chain_table = 1 when the chains come from the back-pointer table, else chain_slices = the
 *   slices of the per-winner redo. */
int vq_index_search_sequence(vq_index* idx, const float* steps /*[m][dim]*/, int m, int k, int64_t min_gap, int64_t max_gap,
                             const int32_t* groups, int32_t n_sel, int exclude,
                             int32_t* groups_out /*[k]*/, float* dist_out /*[k]*/, int32_t* chain_rows /*[k][m] or NULL*/);
int vq_index_search_sequence_device(vq_index* idx, const void* d_steps_f32, int m, int k, int64_t min_gap, int64_t max_gap,
                                    const int32_t* groups, int32_t n_sel, int exclude,
                                    void* d_groups_i32, void* d_dist_f32, void* d_chain_rows_i32 /*or NULL*/);
int vq_debug_sequence_plan(int64_t n, int64_t largest_group, int m, int k, int* step_chunks, int* lds_rows, int* groups_global_form,
                           int64_t* lds_bytes, int* chain_table, int* chain_slices);

/* Span search: per query, the k groups (videos) with the best TIME SPAN — "where in the video does X happen, from when to
 * when?".  Every other search answers with frames or whole videos; a retrieved moment is a start and an end.
 *   Queries q_0 .. q_{nq-1} [nq][dim], used as given, 1 <= nq <= 64.  max_dist tau (fp32; NaN is VQ_ERR_INVALID).  max_gap and
 *   max_span: int64 in position units (vq_index_set_positions), both >= 0 (negative: VQ_ERR_INVALID); values >= 2^32 behave as
 *   2^32 — positions are 32-bit, so that means "no limit".  1 <= k <= 1024.
 *   Gain of a row: d(i, r) = the distance of q_i to row r exactly as vq_index_search reports it (fp32 of the fixed-order fp64
 *   chain); tie(r) = the row number, or the id rank once ranks are set.  w(i, r) = (int64) rint(((double)tau - (double)d(i, r))
 *   * 2^24), rounded to nearest, ties to even, then kept within +-2^31 (a NaN distance takes -2^31).  The fp64 subtraction of
 *   two fp32 values and the scaling by 2^24 are exact, so for distances and tau of ordinary size |w| <= 2^27, and every sum below
 *   is exact in int64.  Integer gains are the point: sums of integers are associative, so a parallel scan in any order gives
 *   the bits of the sequential walk.
 *   Span: s_0 .. s_{L-1} are the rows of group g in (position, tie) order.  A span is an index range [a, b], 0 <= a <= b < L,
 *   with pos(s_{j+1}) - pos(s_j) <= max_gap for every a <= j < b and pos(s_b) - pos(s_a) <= max_span (differences in 64-bit).
 *   Its mass S(a, b) = the sum of w(i, s_j) over j in a..b.  The group's span for query i is the admissible span with S > 0 that
 *   comes first under: largest S; then shortest b - a + 1; then smallest a.  A group with no admissible span of positive mass
 *   has no result for that query and never appears.  The peak is the row of the span with the smallest (d(i, r), tie(r)).
 *   Result per query: D(g) = fp32(-(double)S * 2^-24); the first min(k, allowed groups with a span) groups by (D, label)
 *   ascending.  groups_out [nq][k] int32, dist_out [nq][k] fp32 (D), mass_out [nq][k] int64 or NULL, len_out [nq][k] int32 (the
 *   rows in the span) or NULL, rows_out [nq][k][3] int32 (full-index row numbers of the start, the end and the peak) or NULL.
 *   Unused slots hold -1 / +inf / 0 / 0 / -1.
 *   groups / n_sel / exclude: the host-memory filter of vq_index_search_sequence, with the same two empty-list cases.  Stale or
 *   missing labels, positions or id ranks are refused before any work is queued, as the sequence search refuses them.
 *   Consequences: a group's span does not depend on other groups or on other queries of the call.  max_span = 0 with distinct
 *   positions inside every group: every span is one row, and the groups, their order and their peak rows are those of
 *   vq_index_search_grouped restricted to groups whose best distance is below tau (S = w of that row).  tau so large that every
 *   gain is positive, both limits unlimited: every allowed group's span is all of its rows and S the plain sum.  tau below
 *   every distance: every slot is empty.  Rows whose d equals tau exactly have zero gain and never sit at an end of a returned
 *   span.
 *   How it runs (csrc/knn_span.h): exact only, no mode.  Per chunk of queries the plain search's exact distances [chunk][n]
 *   (chunks keep them within 512 MiB), then one workgroup per (allowed group, query) walks the group's rows in the sequence
 *   search's (position, tie) order (built by the first sequence or span search after the labels, the positions or the id ranks
 *   changed; that one call waits for the stream once).  One pass over 256-row tiles builds the exclusive int64 prefix sums
 *   P[0..L] of the gains, for every end b the first admissible start lo(b) (the larger of a max-scan over the indices behind a
 *   gap above max_gap and a binary search over the sorted positions for max_span) and the prefix minimum of P.  The best start
 *   for b is the index in [lo(b), b] with the smallest P, ties to the largest index: the prefix minimum where lo(b) = 0,
 *   otherwise a range minimum that reads at most 126 + L / 64 entries (64-row block minima, built only when some range needs
 *   them).  The candidates (P[b+1] - P[a(b)], length, a(b)) are reduced over b under the order above.  Groups of at most
 *   4,096 rows keep the arrays in LDS (20 B per row); longer groups run the same arithmetic over global arrays (20 B per row
 *   of the index, only then) with one more level of minima (at most 252 + L / 4096 reads), one workgroup per group that takes
 *   the chunk's queries one after the other.  Each (query, group) files its (D, label) key and (a, b); the clip search's
 *   selection takes the k smallest per query; one workgroup per winner then sums the span's gains again (integers: the same
 *   mass) and finds the peak.  No floating-point arithmetic behind the gain, no global atomics, workgroup barriers only; the
 *   launches queued depend on the shapes only.  Accounted under the existing profile classes (the span kernels under
 *   sequence_dp; VQ_IDX_NCLASS stays 7).
 *   The _device form takes device queries and results, is asynchronous on the index's stream and reads nothing back.
 *   vq_index_last_search_stats afterwards: [0] the (query, group) pairs that hold a span, [1] the allowed groups run by the
 *   global form, [2] the query chunks.
 *   $VQ_AMD_SPAN_LDS_ROWS (the LDS form's row limit, at most 4,096) and $VQ_AMD_SPAN_DIST_BYTES (the distance budget): tests
 *   only, read per call.
 *   vq_debug_span_plan (host only, as vq_debug_sequence_plan): for n rows in n_groups groups whose longest holds largest_group
 *   rows and nq queries — the query chunks, the LDS form's row limit and the dynamic LDS bytes of a group of that many rows
 *   (capped by largest_group), groups_global_form = 1 when the longest group (so at least one) takes the global form, and the
 *   bytes of the global form's scratch (0 without it). */
int vq_index_search_spans(vq_index* idx, const float* queries /*[nq][dim]*/, int nq, int k, float max_dist, int64_t max_gap,
                          int64_t max_span, const int32_t* groups, int32_t n_sel, int exclude,
                          int32_t* groups_out /*[nq][k]*/, float* dist_out /*[nq][k]*/, int64_t* mass_out /*[nq][k] or NULL*/,
                          int32_t* len_out /*[nq][k] or NULL*/, int32_t* rows_out /*[nq][k][3] or NULL*/);
int vq_index_search_spans_device(vq_index* idx, const void* d_queries_f32, int nq, int k, float max_dist, int64_t max_gap,
                                 int64_t max_span, const int32_t* groups, int32_t n_sel, int exclude,
                                 void* d_groups_i32, void* d_dist_f32, void* d_mass_i64 /*or NULL*/, void* d_len_i32 /*or NULL*/,
                                 void* d_rows_i32 /*or NULL*/);
int vq_debug_span_plan(int64_t n, int64_t n_groups, int64_t largest_group, int nq, int* query_chunks, int* lds_rows,
                       int64_t* lds_bytes, int* groups_global_form, int64_t* scratch_bytes);

/* Warped clip alignment: the k groups (videos) that show a clip under a monotone time warp, each with where it starts and ends —
 * "which video contains this clip, played faster, slower or sampled differently, and from where to where?".  vq_index_match_runs
 * reads diagonal runs and so needs equal sampling rates; vq_index_search_sequence joins at most 64 steps, one stored frame each;
 * this is the subsequence dynamic time warp of the clip against every allowed group, with integer costs so that it is exact.
 *   Clip q_0 .. q_{m-1} in time order [m][dim] fp32, used as given, 1 <= m <= 4096.  1 <= k <= 1024.  max_dist: fp32, NaN is
 *   VQ_ERR_INVALID, +inf means no limit.  groups / n_sel / exclude: the host-memory filter of vq_index_search_sequence, with
 *   both of its empty-list cases.  Stale or missing labels, positions or id ranks are refused as the sequence search refuses
 *   them.  Every refusal names the argument in vq_last_error and comes before the device is asked for anything.
 *   Cost of a cell: d(i, r) = the distance of q_i to row r exactly as vq_index_search reports it; c(i, r) = (int64)
 *   rint((double)d(i, r) * 2^24), ties to even, kept within +-2^31; a NaN distance takes +2^31.  The scaling is exact and every
 *   sum below is exact in int64.
 *   Paths: s_0 .. s_{L-1} are the rows of group g in the (position, tie) order the sequence search walks.  A path is a list of
 *   cells (i_t, j_t) with i_0 = 0 and i_last = m - 1 whose every step is (+1, +1), (+1, 0) or (0, +1); its cost C is the sum of
 *   c(i_t, s_{j_t}), its start a = j_0 and its end b = j_last.  Both the start and the end are free.
 *   Best path: cell (i, j) holds the smallest key (C, -a) over the paths that end there — on equal cost the later start wins.
 *   The group's result is the end b with the smallest (C(b), b - a(b) + 1, a(b)), all integers.  D(g) = fp32((double)C * 2^-24 /
 *   (double)m).  A group appears only if D(g) <= max_dist, compared in fp32.  The answer is the first min(k, such allowed
 *   groups) by (C, label) ascending (so dist_out never decreases; two groups whose different costs round to one fp32 D come by
 *   cost).
 *   Alignment: the path of a winner is read back from (m - 1, b).  The predecessor of a cell is the first, in the order diagonal
 *   (i - 1, j - 1), vertical (i - 1, j), [at i = 0: "starts here"], horizontal (i, j - 1), whose key equals the cell's minimum.
 *   align_out [k][m][2] holds, per clip frame, the full-index row numbers of the first and the last stored row paired with it.
 *   Outputs: groups_out [k] int32, dist_out [k] fp32 (D), cost_out [k] int64 or NULL, rows_out [k][2] int32 or NULL (the
 *   full-index rows of s_a and s_b), align_out or NULL.  Unused slots hold -1 / +inf / 0 / -1 / -1.  An empty index returns
 *   every slot empty.
 *   Limit: with align_out, m x (rows of the largest allowed group) x 4 B <= 1 GiB, else VQ_ERR_INVALID; longer clips go in pieces.
 *   Consequences: m = 1 gives the groups and rows of vq_index_search_grouped wherever a group's best distance is unique, with C =
 *   c of that row.  A group of one row: C = the sum over i of c(i, that row) and a = b = 0.  A group's result does not depend on
 *   other groups.  If every c >= 0: C(g) >= the sum over i of min_j c(i, s_j).  Reversing the clip changes the answer.
 *   How it runs (csrc/knn_align.h): exact only, no mode.  Per chunk of clip frames the plain search's exact distances
 *   [chunk][n] (chunks keep them within 512 MiB); the DP row [n] (int64 cost + int32 start, 12 B per row) is carried between
 *   chunks.  One workgroup per allowed group runs the chunk's frames one after the other over the group's rows.  DP row i: P =
 *   the exclusive prefix sums of c(i, .); E(j) = the smaller key of the previous DP row at j - 1 and at j, ties to j - 1 (at i =
 *   0: (0, -j)); cell (i, j) = P[j + 1] + the prefix minimum over j' <= j of (E(j').C - P[j'], -E(j').a, -j') — keys that are
 *   distinct, over 256-row tiles with the running values carried from tile to tile.  Groups of at most 4,096 rows keep the DP
 *   row in LDS (16 B per row: cost, start, row number); longer groups run the same arithmetic on the carried state in global
 *   memory, bit for bit the same.  A small kernel turns the last DP row into each group's (D, label) key, C and (a, b); the clip
 *   search's selection takes the k smallest, and one workgroup per result slot puts the groups that share a D in (C, label)
 *   order, taken over every group that holds that D.  With align_out, one workgroup per winner runs its group's DP again and writes the
 *   entry column j' of every cell (int32, top bit = entered down the diagonal) into a table [m][L], winners batched within
 *   256 MiB (at least one per batch), and one thread per winner walks it back.  No floating point behind the cost, no global
 *   atomics, workgroup barriers only, every loop bounded by the shapes; the launches queued depend on the shapes and the
 *   arguments only.  Accounted under sequence_dp; VQ_IDX_NCLASS stays 7.
 *   The _device form takes device clip and result arrays, is asynchronous on the index's stream and reads nothing back.
 *   vq_index_last_search_stats afterwards: [0] the groups with a result, [1] the allowed groups run by the global form, [2] the
 *   clip chunks.
 *   $VQ_AMD_ALIGN_LDS_ROWS (the LDS form's row limit, at most 4,096), $VQ_AMD_ALIGN_DIST_BYTES (the distance budget) and
 *   $VQ_AMD_ALIGN_BP_BYTES (the winner tables' batch budget): tests only, read per call.
 *   vq_debug_align_plan (host only): for n rows in n_groups groups whose longest allowed one holds largest_group rows, a clip of
 *   m frames and k results — the clip chunks, the LDS form's row limit and the dynamic LDS bytes of a group of that many rows
 *   (capped by largest_group), groups_global_form = 1 when that group takes the global form, the bytes of the carried DP row,
 *   and with with_align the winner batches for min(k, n_groups) winners (0 without).  VQ_ERR_INVALID above the 1 GiB bound. */
int vq_index_align_clip(vq_index* idx, const float* clip /*[m][dim]*/, int m, int k, float max_dist, const int32_t* groups,
                        int32_t n_sel, int exclude, int32_t* groups_out /*[k]*/, float* dist_out /*[k]*/,
                        int64_t* cost_out /*[k] or NULL*/, int32_t* rows_out /*[k][2] or NULL*/, int32_t* align_out /*[k][m][2] or NULL*/);
int vq_index_align_clip_device(vq_index* idx, const void* d_clip_f32, int m, int k, float max_dist, const int32_t* groups,
                               int32_t n_sel, int exclude, void* d_groups_i32, void* d_dist_f32, void* d_cost_i64 /*or NULL*/,
                               void* d_rows_i32 /*or NULL*/, void* d_align_i32 /*or NULL*/);
int vq_debug_align_plan(int64_t n, int64_t n_groups, int64_t largest_group, int m, int k, int with_align, int* clip_chunks,
                        int* lds_rows, int64_t* lds_bytes, int* groups_global_form, int64_t* scratch_bytes, int* winner_batches);

/* Keyframe summary: the k most representative rows of each listed group (video) — the poster frame and thumbnail strip of a
 * video, the few frames that stand in for a long one (as the query set of vq_index_search_set, say).  An iterative
 * farthest-point (greedy k-centre) pass per group: its covering radius is within a factor 2 of the best possible for every k,
 * and its answer for k is a prefix of its answer for k + 1.
 *   Notation: for rows a, b of the index, d(a, b) = 1.0f - fp32(sum_i (double)x_a[i] * (double)x_b[i]), summed in index order:
 *   vq_index_search's distance with row b as the query; symmetric.  tie(r) = the row number, or the id rank once ranks are set.
 *   For one group g (vq_index_set_groups) with rows r_0 < r_1 < .. < r_{L-1} (ascending row number), L >= 1 — the order of the
 *   operations is part of the definition:
 *   1. Mean direction.  The ascending row list is cut into consecutive blocks of 256 rows; per component, B_j[i] = the fp64 sum
 *      of the block's rows in order, each term (double)x[i];  S[i] = B_0[i] + B_1[i] + .. added in fp64 in block order;
 *      c[i] = (float)S[i].  There is no division anywhere (the blocks can run in parallel).
 *   2. Seed.  s_0 = the row of g with the smallest (1.0f - fp32(chain(x_r, c)), tie(r)), the same fp64 chain with c as the
 *      query: the frame most like the video as a whole.
 *   3. State.  near_0(r) = d(r, s_0) and owner_0(r) = 0 for every other row of g.  Chosen rows leave the state for good;
 *      owner(s_t) = t.
 *   4. Radius.  radius[t] = the largest near_t(r) over the rows not yet chosen, 0.0f when none is left: every row of the group
 *      lies within radius[t] of one of the first t + 1 keyframes.
 *   5. Step t + 1.  If t + 1 == k, or no row is left, or radius[t] <= max_radius (an fp32 compare): stop.  Otherwise s_{t+1} =
 *      the row not yet chosen with the largest near_t, the smallest tie among equals; for every other row not yet chosen,
 *      d = d(r, s_{t+1}): if d < near_t(r) (strictly) then near_{t+1}(r) = d and owner_{t+1}(r) = t + 1, else both are kept.
 *   6. Result, with kappa the number of keyframes chosen: rows [0, kappa) = the keyframes in selection order, full-index row
 *      numbers; radius [0, kappa) = the radii; members [t] = the rows of g whose final owner is t (they sum to L).  Unused
 *      slots are -1 / +inf / 0.
 *   Consequences: kappa = min(k, L) when max_radius = -inf; the answer for k is a prefix of the answer for k' > k (rows and
 *   radius; members differ); radius never increases; a group's answer does not depend on any other group; max_radius = rho
 *   returns the shortest prefix whose last radius is <= rho.  Rows that are not finite are outside the definition: such a call
 *   may return anything, but it ends (every loop is bounded by the shapes).
 *   groups [n_sel]: labels of vq_index_set_groups in host memory; duplicates are allowed, each entry is answered on its own
 *   ([n_sel][k] outputs, members_out may be NULL).  A label outside [0, n_groups) is VQ_ERR_INVALID; a label that holds no row
 *   gives empty slots.  Limits: n_sel >= 1, 1 <= k <= 256, max_radius not NaN (-inf: no early stop), else VQ_ERR_INVALID, judged
 *   before the device is asked for.  Stale or missing labels and stale id ranks are refused before any work is queued; no
 *   positions are needed.  An empty index returns every slot empty.
 *   How it runs (csrc/knn_summary.h): exact only.  A listed group of at most 4,096 rows is one workgroup of 256 threads that
 *   runs steps 1 - 6 in one launch: near (as an order-preserving 32-bit key), owner, row and tie per row in LDS (14 B per row,
 *   sized for the longest such group listed, so that several workgroups share a CU), the centre staged in LDS as fp64 once per
 *   step, the pick as the workgroup's maximum of the packed (near key, inverted tie).  Longer groups take the wide form: state
 *   in global memory; per step one update launch over a host-built list of 256-row blocks of all long groups (distance,
 *   min-update, the block's maximum to its own slot) and one pick launch, a workgroup per long group over its blocks' slots
 *   (radius, stop rule, next centre); the mean's block sums run over the same block list.  A group that has stopped sets a
 *   flag and its later blocks return at once; the host never reads between steps.  The launches queued depend on the shapes and
 *   k only: 2, plus 5 + 2 k when a listed group takes the wide form.  No global atomics, no waiting of one workgroup on another.
 *   They are accounted under the existing profile class exact_dist_f64chain (VQ_IDX_NCLASS stays 7).
 *   Scratch: 4 B per listed group and output slot lists; wide form: 8 B per row of the long groups listed, 16 B + dim x 8 B per
 *   256-row block.
 *   The _device form takes device results, is asynchronous on the index's stream and reads nothing back.
 *   vq_index_last_search_stats afterwards: [0] listed groups run by the LDS form, [1] listed groups run by the wide form,
 *   [2] keyframes written.
 *   $VQ_AMD_SUM_LDS_ROWS (tests only, read per call, at most 4,096) lowers the LDS form's row limit.
 *   vq_debug_summary_plan (host only, as vq_debug_sequence_plan): for n rows of dimension dim whose longest listed group holds
 *   largest_group rows — the LDS form's row limit, its dynamic LDS bytes (sized for min(limit, largest_group) rows),
 *   groups_wide_form = 1 when that group (so at least one) takes the wide form, and the launches a call queues. */
int vq_index_summarize_groups(vq_index* idx, const int32_t* groups /*[n_sel]*/, int32_t n_sel, int k, float max_radius,
                              int32_t* rows_out /*[n_sel][k]*/, float* radius_out /*[n_sel][k]*/, int32_t* members_out /*[n_sel][k] or NULL*/);
int vq_index_summarize_groups_device(vq_index* idx, const int32_t* groups /*[n_sel], host*/, int32_t n_sel, int k, float max_radius,
                                     void* d_rows_i32, void* d_radius_f32, void* d_members_i32 /*or NULL*/);
int vq_debug_summary_plan(int64_t n, int64_t largest_group, int dim, int k, int* lds_rows, int64_t* lds_bytes,
                          int* groups_wide_form, int* launches);

/* Zero-shot labelling: given a vocabulary of prompts, which prompt does each row (frame) show, and what is each group (video)
 * about.  Every search above reduces along the row axis, per query; this one reduces along the prompt axis, per row.
 *   Inputs.  Prompts p_0 .. p_{P-1}, 1 <= P <= 4,096, fp32 [P][dim], used as given (HNSWIndex.label_rows normalises them the way
 *   search normalises queries).  d(r, j) = the distance of prompt j to row r exactly as vq_index_search reports it:
 *   1.0f - fp32(sum_i (double)x_r[i] * (double)p_j[i]), summed in index order (oracle/knn_oracle.c).
 *   Row label.  L(r) = the j with the smallest (d(r, j), j): two prompts at equal distance go to the smaller index; id ranks
 *   play no part.  best(r) = d(r, L(r)).  With max_dist (fp32; +inf: off; NaN: VQ_ERR_INVALID) a row with best(r) > max_dist is
 *   unlabelled, L(r) = -1, and best(r) is still reported; best(r) == max_dist stays labelled (an fp32 compare).
 *   Group tags, produced only when group_tags is not NULL (then all four group arrays are needed, and 1 <= m <= 16).  They need
 *   valid group labels (vq_index_set_groups covering every row) and, when id ranks are set, valid ranks: refused like
 *   vq_index_search_grouped otherwise.  votes(g, j) = the number of rows of g with L(r) = j.  The tags of g are the first
 *   min(m, labels with votes > 0) labels by (votes descending, j ascending); tag t carries its votes and show(g, j) = the row of
 *   g labelled j with the smallest (best(r), tie(r)), tie as vq_index_search (the row number, or the id rank): the frame that
 *   shows the tag best.  Unused slots are -1 / 0 / -1.  Unlabelled rows vote for nothing; group_unlabelled [g] counts them.  A
 *   label that holds no row has no tags.
 *   Everything is integers or fp32 values the plain search defines, so the answer is unique.
 *   Refusals (VQ_ERR_INVALID, before any work is queued, the outputs untouched): P or (with group outputs) m out of range;
 *   NaN max_dist; group outputs without valid labels; an unknown mode; mode 2 where the fp16 path does not exist (dim not 256,
 *   512 or 768, or rows that are not near-unit); host form only: a prompt value that is not finite (the device form documents
 *   finite prompts as a precondition: it then still ends, by the exact path, with whatever labels NaN distances give).
 *   An empty index returns 0 and writes nothing.  row_label and row_dist may each be NULL.
 *   Lifetimes.  Labels and ranks are those of vq_index_set_groups / vq_index_set_id_ranks: vq_index_remove_rows compacts both
 *   with the rows (they stay valid); vq_index_update_rows keeps them; rows added afterwards make them stale until they are set
 *   again.  Row labels alone need neither.
 *   How it runs (csrc/knn_label.h, DESIGN.md §4 "Zero-shot labelling").  mode 1, exact: per chunk of prompts (kept within
 *   512 MiB of distances) the tiled fp64-chain distance kernel, then a column arg-min that carries every row's running
 *   (distance, prompt) key across chunks.  mode 2, fp16: one pass over the fp16 matrix per range of 2,048 prompts with the
 *   256 x 256 LDS-DMA mainloop of the clip search, rows and prompts swapped, and an epilogue that keeps every row's three
 *   largest score keys; a row whose best key leads the second by more than 2 E + 2^-19 has a proven label and gets one exact
 *   dot, one that leads the third so gets its two candidates re-scored exactly, any other is filed and redone over all prompts
 *   exactly, on the device.  E = scan_eps_unit(dim) x max |row| x max |p|.  A prompt with |p|^2 outside [0.25, 4] sends the whole
 *   call to the exact path (the host form decides that before queueing, the device form on the device).  mode 0 takes the fp16
 *   path where it exists, the index holds at least 16,384 rows and n x P is at least 2^22 (the measured crossover: below it the
 *   two paths tie or the exact one is ahead).  The [P][n] table never exists on the
 *   fp16 path.  Groups: a group of at most 4,096 rows is one workgroup: an LDS histogram of the labels, m selection rounds, a
 *   second sweep for the show rows.  A longer group is split into pieces of 4,096 rows over workgroups (a histogram per piece,
 *   added in piece order by the group's workgroup, which runs the rounds; then the pieces' show keys, merged in piece order):
 *   four launches for all long groups of a call, P counters per piece (at most 4 B per row of a long group), no [G][P] table.
 *   Scratch: 12 B per row, + 8 B per row (exact) or 20 B per row and prompt range (fp16).
 *   Cost of the device form's flagged call (a prompt norm outside [0.25, 4]): every row is scored against all prompts by one
 *   wave per row, about 3.9e9 exact dots per second at dim 512 on one MI355X (measured through the filed rows of the probe): n
 *   = 1M and P = 4,096 take about a second where the host form's chunked exact path takes 0.25 s.  Normalise the prompts.
 *   The _device form takes device pointers, is asynchronous on the index's stream and reads nothing back.
 *   vq_index_last_search_stats afterwards: [0] rows whose label the fp16 pass proved directly, [1] rows settled by the exact
 *   re-score of their two candidates, [2] rows answered by the exact path over all prompts (mode 1: all of them).
 *   vq_debug_label_plan (host only, near-unit rows assumed; largest_group = the rows of the longest group, 0 without group
 *   outputs): the path (fp16_path), the exact path's chunking, the fp16 path's tiles and scratch, the split form's threshold, piece
 *   length and the pieces of the longest group (0: it runs as one workgroup), and eps: unit rows and prompts whose best and second-best exact scores differ by more than 4 eps are
 *   always proven directly (eps = E for norms up to 1.0001, plus half the slack). */
int vq_index_label_rows(vq_index* idx, const float* prompts /*[P][dim]*/, int P, int mode, float max_dist,
                        int32_t* row_label /*[n] or NULL*/, float* row_dist /*[n] or NULL*/, int m,
                        int32_t* group_tags /*[G][m] or NULL*/, int32_t* group_votes /*[G][m]*/, int32_t* group_show_rows /*[G][m]*/,
                        int32_t* group_unlabelled /*[G]*/);
int vq_index_label_rows_device(vq_index* idx, const void* d_prompts_f32, int P, int mode, float max_dist, void* d_row_label_i32 /*or NULL*/,
                               void* d_row_dist_f32 /*or NULL*/, int m, void* d_group_tags_i32 /*or NULL*/, void* d_group_votes_i32,
                               void* d_group_show_rows_i32, void* d_group_unlabelled_i32);
int vq_debug_label_plan(int64_t n, int dim, int P, int mode, int64_t largest_group, int* fp16_path, int* exact_chunk, int* exact_chunks,
                        int64_t* exact_bytes, int* prompt_tiles, int* prompt_ranges, int64_t* row_tiles, int64_t* part_bytes, float* eps,
                        int* group_split_rows, int* group_piece_rows, int64_t* largest_group_pieces);

/* Library clustering: exact spherical k-means over ALL stored rows; what organises a library nobody has queried yet (the themes
 * of an archive with a poster frame each, material that recurs across videos, a vocabulary for vq_index_label_rows).  The result
 * is a pure function of the rows, the initial centroids and the id ranks: every floating-point operation and its order are part
 * of this definition, and the tests compare bits with a numpy restatement (tests/cluster_ref.py).
 *   Inputs.  P clusters, 1 <= P <= min(4,096, n).  max_iter, 1 <= max_iter <= 1,000.  mode as vq_index_label_rows.  The initial
 *   centroids C_1 come in exactly one of two ways: init, fp32 [P][dim], used as given; or init_rows, int32 [P], C_1[j] = stored
 *   row init_rows[j] (gathered on the device; the same row may be named twice).
 *   Iteration t = 1, 2, ...
 *   1. Assign.  (L_t, best_t) = the row labels and distances of vq_index_label_rows(C_t, max_dist = +inf): its definition
 *      applies, the tie rule included (of two centroids at the same distance the smaller j wins).
 *   2. Stop.  changed[t-1] = the number of rows with L_t != L_{t-1}; changed[0] = n.  The host form stops when t > 1 and
 *      changed[t-1] == 0, or when t == max_iter.
 *   3. Update to C_{t+1}.  For cluster j let R_j be its rows in ascending row number, cnt_j = |R_j|.  R_j is cut into pieces of
 *      1,024 consecutive entries (the last one may be shorter).  piece_sum[i] = the fp64 sum of (double)x_r[i] over the piece's
 *      rows, added one after another in list order, starting from 0.0.  s_j[i] = the pieces' sums added in piece order, starting
 *      from 0.0.  m_j[i] = fp32(s_j[i] / (double)cnt_j).  n2_j = the fp64 sum over i = 0 .. dim-1, in index order, starting
 *      from 0.0, of (double)m_j[i] * (double)m_j[i] (products of two fp32 values are exact in fp64: a fused multiply-add gives
 *      the same sum).  C_{t+1}[j][i] = fp32((double)m_j[i] / sqrt(n2_j)).  If cnt_j == 0 or n2_j == 0, C_{t+1}[j] = C_t[j], bit
 *      for bit.  Every operation is an IEEE fp64 add, divide or square root (round to nearest even), or an exact product.
 *   Result, with T = the last t reached: centroids = C_T [P][dim]; row_label = L_T and row_dist = best_T [n] (either may be
 *   NULL); counts[j] = cnt_j under L_T; show_rows[j] = the row of cluster j with the smallest (best_T, tie), tie as
 *   vq_index_search (the row number, or the id rank), -1 for a cluster without rows; *iterations = T; changed[0 .. T-1] (NULL:
 *   not wanted; the array holds max_iter entries, those from T on are not written).  The labels are always the assignment TO THE
 *   RETURNED centroids: vq_index_label_rows(centroids) reproduces row_label and row_dist bit for bit.
 *   The _device form takes device pointers (d_init or d_init_rows, the other NULL; d_init may be d_centroids itself) and runs
 *   exactly `iters` assignments and iters - 1 updates: no convergence test, nothing read back, asynchronous on the index's
 *   stream.  Past a fixed point every further iteration reproduces the same bits (the update is a pure function of L), so it
 *   agrees with the host form whenever iters >= the host form's *iterations.  Its init_rows entries cannot be checked without
 *   reading them back: entries in [0, n) are a precondition (the gather clamps others into range).
 *   Refused (VQ_ERR_INVALID, before any work is queued, no output touched): P or max_iter / iters out of range; both or neither of
 *   init / init_rows; an init_rows entry outside [0, n) (host form); an init value that is not finite (host form); an unknown
 *   mode, or mode 2 where vq_index_label_rows refuses it; stale id ranks.  An empty index returns 0 and writes nothing.
 *   vq_index_last_search_stats afterwards holds the three label classes of the LAST assignment.
 *   How it runs (csrc/knn_cluster.h, DESIGN.md §4 "Library clustering").  The assignment is the label call's run, unchanged.
 *   The rows are then listed by label in ascending row order (a stable counting sort over blocks of 1,024 rows: integers only);
 *   the same pass counts the changed rows, and the host form reads that one mapped word per iteration.  One workgroup per piece
 *   sums its rows' columns in fp64 (a thread owns four columns; no floating-point atomics anywhere: the order is the
 *   definition), one workgroup per cluster adds the pieces in order and finishes the centroid in place.  The show rows are a
 *   64-bit minimum per cluster over the list, after the last assignment only.  The piece sums are accounted under the profile
 *   class exact_dist_f64chain, the finish under normalize_rows, the list and the show rows under select_topk (VQ_IDX_NCLASS
 *   stays 7).
 *   vq_debug_cluster_plan (host only): the piece length (1,024), the piece kernel's grid max_pieces = floor(n / 1,024) +
 *   min(P, n) (a bound on sum_j ceil(cnt_j / 1,024): workgroups beyond a list's pieces leave at once), the counting sort's blocks
 *   ceil(n / 1,024) and its table (blocks x P x 4 bytes), the pieces' sums (max_pieces x dim x 8 bytes), all scratch, the piece
 *   kernel's threads (dim / 4 rounded up to whole waves) and the launches of one iteration, the assignment aside. */
int vq_index_cluster(vq_index* idx, const float* init /*[P][dim] or NULL*/, const int32_t* init_rows /*[P] or NULL*/, int P, int max_iter,
                     int mode, float* centroids /*[P][dim]*/, int32_t* row_label /*[n] or NULL*/, float* row_dist /*[n] or NULL*/,
                     int32_t* counts /*[P]*/, int32_t* show_rows /*[P]*/, int* iterations, int32_t* changed /*[max_iter] or NULL*/);
int vq_index_cluster_device(vq_index* idx, const void* d_init_f32 /*or NULL*/, const void* d_init_rows_i32 /*or NULL*/, int P, int iters,
                            int mode, void* d_centroids_f32, void* d_row_label_i32 /*or NULL*/, void* d_row_dist_f32 /*or NULL*/,
                            void* d_counts_i32, void* d_show_rows_i32);
int vq_debug_cluster_plan(int64_t n, int dim, int P, int* piece_rows, int64_t* max_pieces, int64_t* list_blocks, int64_t* table_bytes,
                          int64_t* sum_bytes, int64_t* scratch_bytes, int* piece_threads, int* launches);

/* Chapter segmentation: where does a video change subject?  Each listed group (video), walked in time order, is cut into at
 * most k contiguous runs of frames (chapters) so that the frames of a run point the same way: the optimal contiguous
 * k-segmentation under the cost below, by a dynamic programme over a table of pair costs.  The timeline counterpart of the
 * keyframe summary (a thumbnail strip) and of vq_index_cluster (themes across the library).
 *   For one group g (vq_index_set_groups) with L >= 1 rows, let r_0 .. r_{L-1} be its rows in ascending (position, tie) order,
 *   positions as vq_index_set_positions gave them, tie(r) = the row number, or the id rank once ranks are set: the order
 *   vq_index_search_sequence walks.  Parameters k, penalty (fp32), max_len (int64, 0 = none); W = L when max_len = 0, else
 *   min(L, max_len): the longest run allowed.  The order of the operations is part of the definition:
 *   1. Prefix sums.  P_0[i] = 0.0, P_{t+1}[i] = P_t[i] + (double)x_{r_t}[i]: ONE fp64 chain per column along the order (not a
 *      blocked or tree scan).
 *   2. Cost of the run [a, b), 0 <= a < b <= L, b - a <= W.  u[i] = (float)(P_b[i] - P_a[i]): one fp64 subtraction, rounded to
 *      fp32.  V = the fp64 chain over i in index order of (double)u[i] * (double)u[i], from 0.0.  cost(a, b) = (double)(b - a) -
 *      sqrt(V).  (The products of two fp32 values are exact in fp64, so contraction to fma cannot change a bit.)  Its meaning:
 *      the number of frames times the mean cosine distance of the run's frames to the run's mean direction (for unit rows).
 *   3. Dynamic programme.  E_0(0) = 0.0.  For c = 1 .. K, K = min(k, L), and b = c .. L: E_c(b) = E_{c-1}(a*) + cost(a*, b), one
 *      fp64 addition (for c = 1 too), a* = the admissible a with the smallest (E_{c-1}(a) + cost(a, b), a); admissible:
 *      max(c - 1, b - W) <= a < b and E_{c-1}(a) defined.  E_c(b) is undefined when no a is admissible.
 *   4. Number of chapters.  F(c) = E_c(L) + (double)c * (double)penalty (the product is exact).  kappa = the smallest c in 1 .. K
 *      with E_c(L) defined and the smallest F.  No defined E_c(L) (k * W < L): kappa = 0, every slot of the group is empty.
 *   5. Chapters.  The a* followed back from (kappa, L) give chapter t = [a_t, b_t), t = 0 .. kappa - 1 in time order: first =
 *      r_{a_t} and last = r_{b_t - 1} (full-index row numbers), len = b_t - a_t, spread = (float)(cost(a_t, b_t) / (double)len),
 *      show = the row of the chapter with the smallest (1.0f - (float)chain_i((double)x_r[i] * (double)u[i]), tie(r)), u the
 *      chapter's own u: the keyframe summary's seed rule with the chapter as the video.  Per group count = kappa and mean_spread =
 *      (float)(E_kappa(L) / (double)L) (+inf when kappa = 0).  Unused slots are -1 / -1 / 0 / +inf / -1.
 *   Consequences: k = 1 returns the whole video as one chapter; penalty = 0 asks for the best split into at most k parts (more
 *   parts never cost more, up to rounding); a huge penalty returns one chapter; max_len >= L is the same as none; a group's
 *   answer does not depend on any other group.  Rows that are not finite are outside the definition: such a call may return
 *   anything, but it ends (every loop is bounded by the shapes, and every minimum is taken over integer keys).
 *   groups [n_sel]: labels in host memory; duplicates are allowed, each entry is answered on its own ([n_sel] and [n_sel][k]
 *   outputs; show_out and mean_spread_out may be NULL).  A label outside [0, n_groups) is VQ_ERR_INVALID; a label that holds no
 *   row gives empty slots.  Limits, judged before the device is asked for, else VQ_ERR_INVALID naming the argument: n_sel >= 1,
 *   1 <= k <= 64, penalty >= 0 and not NaN, max_len >= 0.  A listed group with L * W > 2^26 pairs is refused with VQ_ERR_INVALID
 *   naming the label: the work is quadratic in the run length, so this is a stated bound (8,192 frames without max_len; any
 *   length with max_len <= 2^26 / L).  Stale or missing labels, positions or id ranks are refused before any work is queued, with
 *   vq_index_search_sequence's lifetime rules.  An empty index returns every slot empty.
 *   How it runs (csrc/knn_segment.h): exact only.  The listed groups are taken in list order in batches whose band tables
 *   (L x W x 8 B per group) stay within 512 MiB, and whose prefix rows ((L + 1) x dim x 8 B) do; per batch four launches: the
 *   prefix kernel (a workgroup per group, a thread per four columns), the pair-cost kernel (a workgroup per 64 x 64 tile of
 *   (a, b) pairs inside the band, all groups of the batch in one grid, prefix rows staged through LDS 32 columns at a time, each
 *   pair's chain owned by one thread) writing cost[b - 1][b - a - 1], the DP kernel (a workgroup per group, E as order-preserving
 *   keys in LDS up to 4,096 rows and in global memory above, back-pointers [K][L + 1] int32 in scratch, the same workgroup picks
 *   kappa and walks back) and the show kernel (a workgroup per group and slot; not queued when show_out is NULL).  One more
 *   launch writes the counters.  The launches depend on the group sizes (known on the host) and the arguments only.  No
 *   floating-point atomics, no global atomics, no waiting of one workgroup on another.  They are accounted under the existing
 *   profile class exact_dist_f64chain (VQ_IDX_NCLASS stays 7).
 *   The _device form takes device results, is asynchronous on the index's stream (once the (position, tie) order is on the
 *   device, as for vq_index_search_sequence) and reads nothing back.
 *   vq_index_last_search_stats afterwards: [0] listed groups that got at least one chapter, [1] pairs costed, [2] group batches.
 *   $VQ_AMD_SEG_COST_BYTES (tests only, read per call) replaces the 512 MiB; $VQ_AMD_SEG_LDS_ROWS (tests only, read per call, at
 *   most 4,096) lowers the DP's LDS row limit.
 *   vq_debug_segment_plan (host only, as vq_debug_summary_plan): for listed groups of lengths[0 .. n_sel) rows in list order — the
 *   batches, the largest batch's table bytes, the DP's LDS row limit and dynamic LDS bytes, global_form = 1 when the longest
 *   listed group keeps E in global memory, the launches a call with show_out queues, and the pairs it costs. */
int vq_index_segment_groups(vq_index* idx, const int32_t* groups /*[n_sel]*/, int32_t n_sel, int k, float penalty, int64_t max_len,
                            int32_t* count_out /*[n_sel]*/, int32_t* first_out /*[n_sel][k]*/, int32_t* last_out /*[n_sel][k]*/,
                            int32_t* len_out /*[n_sel][k]*/, float* spread_out /*[n_sel][k]*/, int32_t* show_out /*[n_sel][k] or NULL*/,
                            float* mean_spread_out /*[n_sel] or NULL*/);
int vq_index_segment_groups_device(vq_index* idx, const int32_t* groups /*[n_sel], host*/, int32_t n_sel, int k, float penalty,
                                   int64_t max_len, void* d_count_i32, void* d_first_i32, void* d_last_i32, void* d_len_i32,
                                   void* d_spread_f32, void* d_show_i32 /*or NULL*/, void* d_mean_spread_f32 /*or NULL*/);
int vq_debug_segment_plan(const int64_t* lengths /*[n_sel]*/, int32_t n_sel, int dim, int k, int64_t max_len, int* batches,
                          int64_t* table_bytes, int* lds_rows, int64_t* lds_bytes, int* global_form, int* launches, int64_t* pairs);

/* Shared-footage search: the k groups (videos) that contain the same footage as a clip, and where — a re-upload, a trailer cut
 * from a film, an intro that opens every episode, a news clip reused in a compilation.  vq_index_search_set is blind to order
 * and reports no span; vq_index_search_sequence takes 64 steps, forces one frame per step and dilutes a partial overlap;
 * vq_index_search_diverse suppresses copies.  This call thresholds the similarity of the WHOLE clip against the WHOLE library
 * and reads diagonal runs off the bits.
 *   Inputs.  Queries q_0 .. q_{m-1} in time order, fp32 [m][dim], used as given (the Python layer normalises them as `search`
 *   does), 1 <= m <= 4096.  max_dist fp32, not NaN (+inf and -inf are allowed).  min_len >= 1, max_miss >= 0, 1 <= k <= 1024.
 *   mode as in vq_index_search_set.  groups / n_sel / exclude: the filter of vq_index_search_set in host memory, with both of
 *   its empty-list cases (n_sel = 0, exclude = 1: unfiltered; n_sel = 0, exclude = 0: every slot empty).
 *   Hit.  d(i, r) = the distance of q_i to row r exactly as vq_index_search reports it: fp32 of the fixed-order fp64 chain.
 *   hit(i, r) holds iff d(i, r) <= max_dist, compared in fp32: inclusive, and a NaN distance never hits.
 *   Runs.  For an allowed group g with rows b_0 .. b_{L-1} in ascending (position, tie) order — the order
 *   vq_index_search_sequence walks — diagonal delta, -(m-1) <= delta <= L-1, is the cells (i, i + delta) with both indices in
 *   range, taken by ascending i.  The diagonal is cut at every stretch of more than max_miss consecutive non-hits and each piece
 *   is trimmed to its first and last hit; each non-empty piece is a RUN with s = its first i, span = last i - first i + 1 and
 *   hits = the hit cells in it.  Runs with hits < min_len are dropped.
 *   Best run of a group: the run with the smallest (-hits, span, delta, s), all integers.  A group with no run never appears.
 *   Answer: the first min(k, groups with a run) allowed groups by (-hits, span, label).  Per slot: group, hits, span, q_first =
 *   s, row_first and row_last = the full-index row numbers of b_{s + delta} and of the last hit cell's row, mean_dist = fp32 of
 *   (the fp64 chain sum of (double)d(i, b_{i + delta}) over the run's hit cells in ascending i) / (double)hits.  Unused slots are
 *   -1 / 0 / 0 / -1 / -1 / -1 / +inf.
 *   Consequences: max_dist = +inf on finite rows makes every cell hit, so the best run of g has hits = span = min(m, L) on the
 *   smallest delta among the diagonals of that length: delta = min(0, L - m); max_dist = -inf returns nothing; m = 1 with min_len =
 *   1 returns exactly the allowed groups whose vq_index_search_grouped best distance is <= max_dist, in label order.
 *   Limits, judged before the device is asked for anything, else VQ_ERR_INVALID naming the argument: the ranges above, and
 *   m x ceil(n / 32) x 4 B <= 512 MiB for the bit table (m = 4,096 at a million rows: a stated bound, like the segmentation's
 *   pair bound; a longer clip goes in pieces).  Stale or missing labels, positions or id ranks are refused with
 *   vq_index_search_sequence's lifetime rules; mode 2 where the tile path does not exist (dim not 256, 512 or 768, rows that are
 *   not near-unit) is refused too.  An empty index returns every slot empty.
 *   How it runs (csrc/knn_match.h, DESIGN.md §4 "Shared footage").  The answer is a function of the hit bits alone, so both
 *   paths fill one bit table [m][ceil(n / 32)] and share everything behind it.  mode 1, exact: per chunk of queries the plain
 *   search's exact distances [chunk][n] (within 512 MiB) and a kernel that packs d <= max_dist 32 rows to a word.  mode 2, tile
 *   path: the 256-query x 2,048-row workgroup of the clip search's fp16 pass over the fp16 matrix, whose epilogue classifies
 *   every score against T = 1 - max_dist: above T + E_i + slack a sure hit, below T - E_i - slack a sure miss (E_i =
 *   scan_eps_unit(dim) x max|row| x |q_i|, slack 2^-19), otherwise the pair (i, r) is appended to a filed list (64-bit integer
 *   cursor, 16M pairs); whole bit words leave by plain stores and no [m][n] score table exists; a second kernel decides every
 *   filed pair by the exact chain and sets its bit by an integer atomicOr.  A query with |q|^2 outside [0.25, 4] (or not finite)
 *   or a filed list that overflows sets the call's flag to 2 and the exact chain then rewrites the whole table on the device
 *   (the host form sees such a query before it queues anything and takes the chunked exact path, reporting the same flag).
 *   mode 0 takes the tile path where it exists from 16,384 rows and 32 clip frames.  Then one thread per diagonal of every
 *   allowed group walks its bits through the (position, tie) order and the group's best run is kept as one 64-bit integer key
 *   (a workgroup reduction, then an integer atomicMin per group); a small kernel builds each group's (-hits, span, label) key,
 *   the clip search's selection takes the k smallest, and one workgroup per winner recomputes its hit cells' distances by the
 *   chain for mean_dist.  No floating-point atomics, no waiting of one workgroup on another, every loop bounded by the shapes;
 *   the launches depend on the shapes and the arguments only.  Accounted under the existing profile classes (VQ_IDX_NCLASS
 *   stays 7): the tile kernel under scan_f16_mfma_top2, the run pass under sequence_dp.
 *   The _device form takes device queries and results, is asynchronous on the index's stream (once the (position, tie) order is
 *   on the device, as for vq_index_search_sequence) and reads nothing back.
 *   vq_index_last_search_stats afterwards: [0] groups with a run, [1] pairs filed (0 on the exact path and for a flagged call),
 *   [2] the flag (0, or 2 when the exact chain answered a tile-path call).
 *   $VQ_AMD_MATCH_FILED_CAP (tests only, read per call) lowers the filed list's capacity.
 *   vq_debug_match_plan (host only, near-unit rows assumed, as vq_debug_segment_plan): the path, the bit table's bytes (above the
 *   bound: VQ_ERR_INVALID), the exact path's query chunks, the tile path's query tiles, row ranges and workgroups, the filed
 *   capacity, the bits the run key uses (at most 63), the run pass's workgroups and the kernels a call queues. */
int vq_index_match_runs(vq_index* idx, const float* queries /*[m][dim]*/, int m, int k, float max_dist, int min_len, int max_miss, int mode,
                        const int32_t* groups, int32_t n_sel, int exclude,
                        int32_t* groups_out /*[k]*/, int32_t* hits_out /*[k]*/, int32_t* span_out /*[k]*/, int32_t* q_first_out /*[k]*/,
                        int32_t* row_first_out /*[k]*/, int32_t* row_last_out /*[k]*/, float* mean_dist_out /*[k]*/);
int vq_index_match_runs_device(vq_index* idx, const void* d_queries_f32, int m, int k, float max_dist, int min_len, int max_miss, int mode,
                               const int32_t* groups, int32_t n_sel, int exclude,
                               void* d_groups_i32, void* d_hits_i32, void* d_span_i32, void* d_q_first_i32, void* d_row_first_i32,
                               void* d_row_last_i32, void* d_mean_dist_f32);
int vq_debug_match_plan(int64_t n, int64_t n_groups, int dim, int m, int mode, int* fp16_path, int64_t* bits_bytes, int* exact_chunk,
                        int* exact_chunks, int* q_tiles, int* ranges, int64_t* tile_grid, int64_t* filed_cap, int* key_bits,
                        int64_t* run_blocks, int* launches);

/* Library neighbours: for every asked row of the index its k nearest stored rows among the rows that are not "the same" as it.
 * Every other search starts from a query the caller brings; this one answers the library's questions about itself (which frames
 * also exist in another video, which videos are related, "more like this frame, elsewhere") from one table.
 *   Inputs.  rows: m row numbers in host memory (read before the call returns), in any order, repeats allowed: every entry gets
 *   its line; NULL = every row in row order, and m must then be the index's size.  An entry outside [0, size) is VQ_ERR_INVALID.
 *   m = 0 is a no-op.
 *   Eligible set of an asked row r.  exclude = 0: S(r) = { c : c != r }.  exclude = 1: S(r) = { c : group(c) != group(r) }, which
 *   needs current labels (vq_index_set_groups): stale or missing labels are VQ_ERR_INVALID before anything is queued, as in the
 *   grouped search.
 *   Result.  Line r of ids / dist [m][k] holds the first min(k, |S(r)|) rows of S(r) by (d(r, c), tie(c)) ascending, where
 *   d(r, c) = fp32(1 - fp32(dot(row_c, row_r))) by the fixed-order fp64 chain of vq_index_search with the stored fp32 master of
 *   row r as the query, used as given, and tie(c) is the row number, or the id rank once vq_index_set_id_ranks was called.
 *   Unused slots are -1 / +inf.  So with exclude = 1 line r is bit for bit what vq_index_search_filtered(query = master row r,
 *   groups = {group(r)}, exclude = 1) returns, and with exclude = 0 it is vq_index_search(row r, k + 1) with r struck out.
 *   Modes follow vq_index_search.  1: exact, 1 <= k <= 1024.  2: fp16 tile scan with the matrix on both sides (per-pair mask),
 *   exact re-score with proof, exact redo on the device for the rows the proof leaves open; k <= 100; refused with
 *   VQ_ERR_INVALID unless dim is 256, 512 or 768 and the rows are near-unit.  0: the library's choice (mode 2 from 16,384 stored
 *   rows and 64 asked rows, when mode 2 would be accepted).
 *   The _device form takes device result pointers (rows stays host memory) and is asynchronous on the index's stream.
 *   vq_index_last_search_stats afterwards reports [0] rows proven on the fp16 path, [1] rows of [0] that needed stream rescans,
 *   [2] rows answered exactly.
 *   $VQ_AMD_NEIGHBORS_CHUNK (tests only, read per call) replaces the number of asked rows per chunk, rounded up to 256.
 *   vq_debug_neighbors_plan: the plan for near-unit rows, pure arithmetic, no device: chunk_rows asked rows per chunk (whole
 *   256-row tiles within the key budget on the fp16 path, within 512 MiB of distances on the exact path), the chunk count, the
 *   bytes of keys per chunk (0 on the exact path), the re-score kernel's candidate pool (0: 32 candidates, k <= 20; 1: 80, k <= 64; 2: 128,
 *   k <= 100; four rows per workgroup, up to 8, 8 and 6 stream rescans per row) and eps: rows whose k-th and (k+1)-th eligible scores differ by more than 4 eps are proven. */
int vq_index_neighbors(vq_index* idx, const int64_t* rows, int64_t m, int k, int exclude, int mode, int32_t* ids, float* dist);
int vq_index_neighbors_device(vq_index* idx, const int64_t* rows, int64_t m, int k, int exclude, int mode, void* d_ids_i32,
                              void* d_dist_f32);
int vq_debug_neighbors_plan(int64_t n, int dim, int64_t m, int k, int exclude, int mode, int* fp16_path, int64_t* chunk_rows,
                            int64_t* chunks, int64_t* key_bytes, int* rescore_kind, float* eps);

/* Compound search: the k best rows that match ALL of several prompts — "a dog AND a beach, in the same frame, but NOT at night".
 * Adding the prompt vectors ranks by the SUM of the similarities: a frame that shows one term very well and the other not at all
 * beats a frame that shows both.  Here a frame's WORST required term decides its place.
 *   Inputs.  Terms q_0 .. q_{m-1}, 1 <= m <= 16, fp32 [m][dim], used as given (the Python layer normalises them as `search`
 *   normalises queries).  clause_of[j] (int32, host memory, read before the call returns) is a clause number in [0, C) or -1 for a
 *   veto term; the clause numbers do not decrease over the non-veto terms and every value 0 .. C-1 occurs; C >= 1.  margin is
 *   fp32; -inf and +inf are allowed.
 *   Definition (the order of operations is part of it).  d(j, r) = the distance of term j to row r exactly as vq_index_search
 *   reports it: fp32(1 - fp32(dot)), the dot by the index-order fp64 chain.  Clause value c_i(r) = min over the terms j of clause
 *   i of d(j, r): any alternative satisfies the clause.  Row distance D(r) = max over the clauses i of c_i(r): every clause must
 *   be satisfied and the worst one decides.  Both are fp32 comparisons of values the plain search defines: no new rounding.
 *   Veto: row r is struck iff some veto term j has d(j, r) < fp32(D(r) + margin) — one fp32 addition and a strict compare.
 *   margin = 0 strikes a frame that shows the unwanted prompt better than it shows the wanted combination (the nearest-prompt
 *   rule of vq_index_label_rows: no calibrated threshold needed); margin = -inf strikes nothing; margin = +inf everything.
 *   Answer: the first k rows that are not struck by (D, tie) ascending, tie as in vq_index_search (the row number, or the id rank
 *   once vq_index_set_id_ranks is set): ids [k] row numbers, dist [k] their D; unused slots are -1 / +inf.  term_dist [k][m] (may
 *   be NULL) holds d(j, ids[t]) for every result, +inf in unused slots: it tells which term held a frame back.  Everything is an
 *   fp32 value the plain search defines, or an integer, so the answer is unique.
 *   Consequences: m = 1 with one clause is vq_index_search(nq = 1) bit for bit in every mode; one clause of m terms (pure OR)
 *   is the merge of the m plain exhaustive lists, one entry per row; repeating a term in a second clause changes nothing; a veto
 *   term bit-equal to a term that forms a one-term clause of its own, at margin 0, keeps exactly the rows whose D that term
 *   decides; margin = -inf with veto terms equals the call without them.
 *   Refusals (VQ_ERR_INVALID, before any work is queued, the outputs untouched): m outside [1, 16]; k outside [1, 1024]; a
 *   malformed clause_of (a value below -1 or >= m, a decreasing sequence, a gap in the numbering, veto terms only); NaN margin; an
 *   unknown mode; stale id ranks, as vq_index_search refuses them; mode 2 where the fp16 path does not exist (dim not 256, 512 or
 *   768, rows that are not near-unit, k > 100); host form only: a term value that is not finite (the device form documents finite
 *   terms as a precondition: it then still ends, by the exact path).  An empty index returns 0 with every slot empty.
 *   How it runs (csrc/knn_compound.h, DESIGN.md §4 "Compound search").  mode 1, exact: one tiled fp64-chain kernel writes the
 *   [m][n] term distances (a table of its own, at most 64 MiB per million rows) and the combined row D, +inf where struck; the
 *   plain search's exact selection runs on that row; a last kernel reads the winners' term distances from the table and empties
 *   the slots of struck rows.  mode 2, fp16: ONE read of the fp16 matrix by the streaming scan with the terms as its 16 query
 *   columns; the term axis is reduced per row in registers (max within a clause, min over the clauses, a conservative veto test)
 *   before the per-stream top-2 fold, so the keys are those of one virtual query; one workgroup re-scores the best 32 .. 128 keys
 *   exactly (m fp64 chains each, the veto decided exactly) and proves that no other row can reach the k-th survivor: every bound
 *   + E + 2^-20 must lie below its score, E = scan_eps_unit(dim) x max |row| x max_j |q_j|.  A call that is not proven (a term
 *   with |q|^2 outside [0.25, 4]; too many tied keys; more than four streams whose unseen rows could matter — up to four are
 *   re-scored in full, the largest key first; a veto that leaves the pool short) is redone
 *   by the exact path on the device behind one flag.  mode 0 takes the fp16 path where it exists, from 262,144 rows (the measured
 *   crossover: the one-workgroup re-score costs more than the plain search's) and k <= 100.
 *   The _device form takes device pointers for the terms and the results (clause_of stays on the host), is asynchronous on the
 *   index's stream and reads nothing back.  vq_index_last_search_stats afterwards: [0] 1 if the fp16 path proved the answer,
 *   [1] rows re-scored exactly, [2] 1 if the exact path answered.
 *   vq_debug_compound_plan (host only, near-unit rows assumed, m one-term clauses): the path, the key streams of the scan, the
 *   re-score pool (0 on the exact path), the bytes of the exact path's term table, and eps: unit rows and terms whose k-th and
 *   (k+1)-th exact D differ by more than 4 eps are always proven when the k best rows reach the pool (eps = E for norms up to
 *   1.0001, plus half the slack). */
int vq_index_search_compound(vq_index* idx, const float* terms /*[m][dim]*/, int m, const int32_t* clause_of /*[m], host*/, float margin,
                             int k, int mode, int32_t* ids /*[k]*/, float* dist /*[k]*/, float* term_dist /*[k][m] or NULL*/);
int vq_index_search_compound_device(vq_index* idx, const void* d_terms_f32, int m, const int32_t* clause_of /*[m], host*/, float margin,
                                    int k, int mode, void* d_ids_i32, void* d_dist_f32, void* d_term_dist_f32 /*or NULL*/);
int vq_debug_compound_plan(int64_t n, int dim, int m, int k, int mode, int* fp16_path, int64_t* streams, int* rescore_pool,
                           int64_t* exact_bytes, float* eps);

/* save / load support (hnsw.py:306-380): the stored (normalised) rows. */
int vq_index_export(vq_index* idx, float* rows /*[size][dim]*/);
/* Single stored rows (the reference reads `self.data[node_id]`, a dict lookup): out [n][dim] = rows row_numbers[0..n). */
int vq_index_read_rows(vq_index* idx, const int64_t* row_numbers, int64_t n, float* out);

/* ---- multi-GPU exchange over RCCL (xGMI): one process per GPU ------------------------------------
 * The reference is single-device; these entry points are what a multi-GPU deployment of its
 * ingest loop (src/video_search_system.py:152-181) and of its search (:297) adds: an all-gather of the per-shard
 * embeddings before indexing, and for a row-sharded matrix an all-gather of the per-shard top-k followed by a
 * k-way merge in the reference's (distance, id) order (src/indexes/hnsw.py:269).  librccl is loaded on first
 * use.  Rank 0 makes the id (vq_comm_unique_id, 128 bytes) and ships it to the other ranks by any side
 * channel (torch.distributed's store, a file, MPI); every rank then calls vq_comm_init after vq_init. */
typedef struct vq_comm vq_comm;
#define VQ_COMM_ID_BYTES 128
int vq_comm_unique_id(void* out_id, int bytes);
int vq_comm_init(int rank, int world, const void* unique_id, vq_comm** out);
int vq_comm_destroy(vq_comm* comm);
int vq_comm_info(vq_comm* comm, int* rank, int* world, int* rccl_version);
/* Collectives and failures.  Every rank must make the same sequence of calls with the same counts / nq / k.  No call leaves a
 * rank waiting in a collective its peer never enters: argument checks that fail alike on every rank come first; a call
 * that needs more scratch than the ranks have agreed on allocates and then exchanges ONE status word per rank (an
 * allocation that failed anywhere makes every rank return an error before the data collective; steady-state calls skip
 * this); a failure that can strike one rank only after that point is carried INTO the collective as a status word (below). */
/* counts[world]: rows each rank contributes (this rank's d_local holds counts[rank] x dim fp32); d_out receives
 * sum(counts) x dim in rank (= frame) order on every rank.  Asynchronous on hip_stream, except for the call that first
 * needs (more) padding scratch for ragged counts: that one waits for the stream once (status exchange). */
int vq_allgather_rows(vq_comm* comm, const void* d_local, const int64_t* counts, int dim, void* d_out, void* hip_stream);
/* The ragged all-gather's second half on its own: d_padded [world][pad_rows][dim] fp32 -> the first counts[r] rows of every
 * rank's block, back to back, at d_out.  Asynchronous on hip_stream. */
int vq_compact_gathered_rows(const void* d_padded, const int64_t* counts, int world, int64_t pad_rows, int dim, void* d_out,
                             void* hip_stream);
/* This rank's index holds rows [row_offset, row_offset + size) of the global matrix.  Same modes and result
 * layout as vq_index_search_device, ids are GLOBAL row numbers, identical on every rank.  world*k <= 1024.
 * A rank whose LOCAL scan fails (its shard refuses the requested mode, stale id ranks, a launch error, a row_offset its
 * shard overflows) returns that error — after entering the exchange with empty keys and a non-zero status word.  On its
 * peers the call itself returns 0 (it is asynchronous), every result slot comes back empty (id -1, +inf) and
 * vq_comm_check reports the failed rank once the stream has been synchronised.  Ties across shards are ordered by global
 * row number (vq_index_set_id_ranks orders ties inside a shard only). */
int vq_index_search_sharded(vq_index* idx, vq_comm* comm, const void* d_queries_f32, int nq, int k, int mode,
                            int64_t row_offset, void* d_ids_i32, void* d_dist_f32);
/* 0, or VQ_ERR_STATE once after a sharded search on this communicator was voided by a peer's local failure. */
int vq_comm_check(vq_comm* comm);
/* The merge step alone: [world][nq][k] shard results with global ids (-1 / +inf = empty slot) -> [nq][k]. */
int vq_merge_topk_device(const void* d_all_ids_i32, const void* d_all_dist_f32, int world, int nq, int k,
                         void* d_ids_i32, void* d_dist_f32, void* hip_stream);

/* Device timing of the scan kernels between begin/end (bench.py roofline leg). */
#define VQ_IDX_NCLASS 7
int vq_index_profile_begin(vq_index* idx);
int vq_index_profile_end(vq_index* idx, float* ms /*[VQ_IDX_NCLASS]*/, int* launches /*[VQ_IDX_NCLASS]*/);
const char* vq_index_profile_class_name(int cls);
/* counters of the last fp16-scan search: [0] queries verified exact by the
 * margin test, [1] queries that needed block rescans, [2] queries sent to the
 * full exact scan.  After vq_index_search_grouped*: [0] queries answered by the
 * fp16 path, [1] candidate rows re-scored exactly (summed over queries), [2]
 * queries answered by the exact path. */
int vq_index_last_search_stats(vq_index* idx, int64_t* stats /*[3]*/);

/* What an fp16 search (mode 2) of nq queries for k results over n rows of dimension dim would launch (csrc/scan_plan.h), in
 * this build and with this process's environment switches; force_scan != 0 takes the place of $VQ_AMD_SCAN.
 * scan: 1 the 128 x 1024 MFMA tile, 3 the streaming scan of small batches, 5 the 256 x 2048 batch scan (2, 4: its superseded
 * predecessors, `make EXPERIMENTS=1`; 51-53: diagnostic forms of 5, `make DIAG=1`).  qt / range: queries / rows per scan
 * workgroup; streams = n_pad / 128 keys pairs per query; q_chunk queries per chunk (1 GiB of keys), `chunks` of them.
 * nqg, fused_q: the streaming scan's groups of 16 queries per pass, and whether it rounds the queries itself (no
 * conversion launch).  rescore: 0 BATCH8, 1 LARGE4, 2 XLARGE4, 3 LARGE1, 4 XLARGE1, 5 SMALL32, 6 SMALL64, with its queries
 * per workgroup, dynamic LDS and the key layout it is told (1, 2, 3); rescore_files_flags: its workgroup writes the flagged
 * list and the counters itself (no collect_flags_kernel).  q_pad .. rescore_grid: the launch of the first (largest) chunk.
 * Pure host arithmetic: needs neither vq_init nor a device.  A scan this build does not carry returns VQ_ERR_INVALID. */
typedef struct vq_scan_plan {
    int64_t scan, qt, range, n_pad, streams, ranges, q_chunk, chunks, nqg, fused_q, rb, scan_lds;
    int64_t rescore, rescore_qpw, rescore_lds, layout, rescore_files_flags;
    int64_t q_pad, q_tiles, scan_grid_x, scan_grid_y, rescore_grid;
} vq_scan_plan;
int vq_debug_scan_plan(int dim, int64_t n, int nq, int k, int force_scan, vq_scan_plan* out);

/* Stage read-back of the fp16 scans (tests/test_scan_stages.py): what pass 1 of the last fp16 search left on the device,
 * before any re-score.  Both calls wait for the handle's stream, copy, and change nothing; no search launches or waits
 * anything for them (the handle only remembers the geometry of its last scan).  VQ_ERR_STATE when no such search has run on
 * the handle since its rows last changed (vq_index_add*, _update_rows, _remove_rows, _clear).
 *   vq_index_debug_read_scan_keys: after vq_index_search* in mode 2 (or mode 0 where it took the fp16 path), or after
 *   vq_index_search_filtered* where it took the masked fp16 path (info[4] = 1).  The keys of the LAST chunk of that search:
 *   info = {q0, cur, layout, streams, masked}: the chunk covered queries q0 .. q0 + cur - 1; layout 1, 2 or 3 as in
 *   vq_scan_plan; streams = key pairs per query.  keys [cur][streams][2]: the raw 32-bit patterns, first and second key of
 *   every (query, stream), gathered through the offset functions the re-score kernels read them with.  A key is the fp32
 *   score of one row of the stream with the row's index inside the stream in its low 7 bits (vq_debug_scan_row_of gives the
 *   row number); "no row" (a row past the end, a disallowed row, a stream the masked scan did not read) reads as a float
 *   below -1e38.  keys == NULL: info only.  capacity: the words `keys` holds; fewer than cur * streams * 2 is
 *   VQ_ERR_INVALID.
 *   vq_index_debug_read_group_best: after vq_index_search_grouped* or vq_index_search_grouped_filtered* where they took the
 *   fp16 path.  info = {q0, cur, n_groups}; best [cur][n_groups]: the largest fp16 score the group-max scan saw for the
 *   (query, group), decoded from its order-preserving key to a float.  A group no (allowed) row was seen for reads as NaN:
 *   its key is 0, which no score encodes (a score's key is never 0, and a scan never produces a NaN score from finite
 *   rows and queries).  best == NULL: info only.
 *   vq_debug_scan_row_of: the row number of index `local` (0 .. 127) of stream `stream` under key layout 1, 2 or 3, by
 *   the functions the re-score kernels use; -1 for any other argument.  Pure host arithmetic: no device.
 *
 * The streamed 256 x 256 tile scans (tests/test_tile_scan_stages.py) are read back the same way:
 *   vq_index_neighbors in mode 2 leaves its LAST chunk's keys for vq_index_debug_read_scan_keys: layout 2, streams = the
 *   plan's, q0 / cur = that chunk's asked rows, info[4] = 2: eligibility by tag (a struck pair reads as "no row").
 *   vq_index_search_set where it took the fp16 path leaves its LAST query chunk's maxima for vq_index_debug_read_group_best,
 *   whichever of the two group-max scans wrote them (nothing behind the scan writes that buffer).
 *   vq_index_debug_group_scan_kind says which: info = {kind, chunks, tile_chunks}, kind 1 = the grouped search's streaming
 *   scan, 2 = the clip search's streaming scan (a chunk of at most 16 queries), 3 = set_group_max_kernel; chunks = the query
 *   chunks of the call that left the record, tile_chunks = how many of them ran set_group_max_kernel.
 *   vq_index_debug_read_label_parts: after a labelling call that took the tile path and was not flagged (flagged:
 *   VQ_ERR_STATE).  info = {n, n_pad, ranges, P}; parts [ranges][5][n_pad]: per (prompt range, row) the words k1, j1, k2, j2, f
 *   as label_tile_kernel wrote them: keys are order-preserving words of the fp32 score with the inverted lane-local prompt
 *   index in the low 7 bits, 0 = nothing; j1, j2 the prompt numbers (-1: none).  Rows from n to n_pad are pad rows.
 *   vq_index_debug_read_match_bits: after a shared-footage call that took the tile path.  info = {m, W, n, cursor, flag, cap};
 *   bits [m][W]: the FINAL hit-bit table (tile kernel, patch and, when flag == 2, the exact redo); filed: the first
 *   min(cursor, cap) entries of the filed list, (query << 32) | row, in the order the atomics gave them.  Either array may be
 *   NULL. */
int vq_index_debug_read_scan_keys(vq_index* idx, int64_t* info /*[5]*/, uint32_t* keys, int64_t capacity);
int vq_index_debug_read_group_best(vq_index* idx, int64_t* info /*[3]*/, float* best, int64_t capacity);
int vq_index_debug_group_scan_kind(vq_index* idx, int64_t* info /*[3]*/);
int vq_index_debug_read_label_parts(vq_index* idx, int64_t* info /*[4]*/, uint32_t* parts, int64_t capacity);
int vq_index_debug_read_match_bits(vq_index* idx, int64_t* info /*[6]*/, uint32_t* bits, int64_t bits_capacity, uint64_t* filed,
                                   int64_t filed_capacity);
int64_t vq_debug_scan_row_of(int layout, int64_t stream, int local);

/* Stage entry of the fp16 re-score (tests/test_rescore_stages.py): pass 2 of an fp16 search on a key table the CALLER wrote.
 * It plans as vq_index_search(mode = 2) does for (nq, k) over the handle's rows, under the same preconditions (dim % 64 == 0,
 * k <= 100, a non-empty index of near-unit rows, id ranks that cover the index or none), scatters `keys` [nq][streams][2]
 * (streams and the layout as in vq_scan_plan; the words as vq_index_debug_read_scan_keys returns them) into the key buffer
 * through the plan layout's offset function, the query slots from nq to q_pad holding "no row", uploads the queries and makes
 * the re-score launch of the search: the same function, the same kernel choice.  Nothing else is launched: no conversion,
 * no scan, no flag collection, no exact fallback (a one-query launch of the 32- or 64-candidate kernel files its own flagged
 * slot and counters, as in the search).  It waits and returns what pass 2 left: ids and dist [nq][k], flags [nq] (0 proven
 * exact, 1 proven exact after stream rescans, 2 not proven: the search would redo the query exactly, and ids / dist of such a
 * query mean nothing).  Afterwards vq_index_debug_read_scan_keys returns the table just written; the search statistics are not
 * touched.  nq must fit one chunk of the plan (VQ_ERR_INVALID otherwise); capacity: the words `keys` holds.
 * THE CONTRACT a table must meet for flags 0 / 1 to mean "exact" (what tests/scan_stage_ref.py::check_keys asserts of a scan),
 * with E = scan_eps_unit(dim) x max(1, largest |row|) x |q|, for every (query, stream):
 *   - a key that names a row (a float above -1e38; the row is vq_debug_scan_row_of(layout, stream, key & 127), below the row
 *     count) lies within E of that row's exact score; the two keys of a stream name different rows;
 *   - key1 >= key2; a stream with one row has one such key, a stream with none has none;
 *   - every row of the stream that neither key names scores at or below key2 + E.
 * A table outside the contract is the caller's problem: the kernels stay inside their buffers for ANY words (a key whose row
 * lies past the end is skipped), but what they prove about such a table is not a statement about the rows. */
int vq_index_debug_rescore(vq_index* idx, const float* queries /*[nq][dim], host*/, int nq, int k,
                           const uint32_t* keys /*[nq][streams][2], host*/, int64_t capacity,
                           int32_t* ids /*[nq][k]*/, float* dist /*[nq][k]*/, int32_t* flags /*[nq]*/);

/* Stage entry of the clustering update (tests/test_cluster.py): the update step of vq_index_cluster alone, on labels the CALLER
 * wrote.  labels [n] (host, each in [0, P), VQ_ERR_INVALID otherwise; a non-empty index) take the place of an assignment;
 * centroids_in [P][dim] are C_t.  It builds the by-label list and runs the piece sums and the finish, the launches of the loop
 * through its own functions, waits, and returns C_{t+1} and the clusters' row counts.  The search statistics are not touched. */
int vq_index_debug_cluster_update(vq_index* idx, const int32_t* labels /*[n], host*/, int P, const float* centroids_in /*[P][dim], host*/,
                                  float* centroids_out /*[P][dim]*/, int32_t* counts /*[P]*/);

/* Stage entry of the exact redo (tests/test_exact_stages.py): pass 3 of an fp16 search on flags the CALLER wrote.
 *   vq_debug_fallback_plan: the redo's geometry for n rows, nq queries and k results, out = {fast_splits, fast_rows, splits,
 *   rows, round_q, partial}: the row splits and rows per split of the first round (the first 64 flagged queries) and of a bulk
 *   round, the flagged queries a bulk round takes, and the 8-byte keys of scratch that holds both rounds' per-split lists.
 *   1 <= n < 2^31, nq >= 1, 1 <= k <= 100.  Pure host arithmetic: needs neither vq_init nor a device.
 *   vq_index_debug_fallback: under the preconditions of vq_index_debug_rescore (dim % 64 == 0, k <= 100, a non-empty index of
 *   near-unit rows, id ranks that cover the index or none) it uploads `ids` and `dist` [nq][k] as the answer passes 1 and 2
 *   would have left, then `flags` [nq] (0 and 1: proven; every other value counts as 2: redo) and the queries, and makes the
 *   two launches that end the search: the flag collection and the exact redo, through the search's own function.  Nothing
 *   else is launched: no conversion, no scan, no re-score.  groups == NULL (n_sel = 0): the unmasked redo of
 *   vq_index_search.  Otherwise groups / n_sel / exclude are a filter as in vq_index_search_filtered (labels set and
 *   covering the index) and the redo is the masked one of the masked fp16 path, under the same bitmap; unlike that search
 *   it takes any dim % 64 == 0 and any nq, since no masked scan runs.  An empty exclude list is the unmasked redo, as in the
 *   search; a filter that allows no row is VQ_ERR_INVALID.  It waits and returns ids and dist: a flagged query's slots hold
 *   its exact k best allowed rows by (distance, id), -1 / +inf behind the last one; every other slot holds the caller's bits
 *   untouched.  counters = {flagged, flags == 0, flags == 1, flags counted as 2}.  The search statistics and what
 *   vq_index_debug_read_scan_keys returns are not touched. */
int vq_debug_fallback_plan(int64_t n, int nq, int k, int64_t* out /*[6]*/);
int vq_index_debug_fallback(vq_index* idx, const float* queries /*[nq][dim], host*/, int nq, int k, const int32_t* flags /*[nq], host*/,
                            const int32_t* groups, int32_t n_sel, int exclude, int32_t* ids /*[nq][k], in and out*/,
                            float* dist /*[nq][k], in and out*/, int32_t* counters /*[4]*/);

/* ------------------------------------------------------------------ frame preprocessing
 * The resize in front of the encoder, bit-identical to Pillow's 8-bit separable resample
 * (Pillow src/libImaging/Resample.c), which is what the reference runs in two places:
 *   - transforms.Resize((224, 224)) on a PIL image, feature_extractor.py:54-61, :105-116
 *       -> filter BILINEAR, out 224x224, crop = the whole resized frame;
 *   - CLIPProcessor on the live path, video_search_overhaul.py:129-135, :218-221, :283-289
 *       -> filter BICUBIC, short edge to 224, centre crop 224x224 (vq_clip_processor_geometry).
 * Frames are uint8 [n][h][w][3] of one size; channel order is untouched (resize is per channel).
 * The resized frame is out_h x out_w; only the window crop_h x crop_w at (crop_top, crop_left) is produced:
 * out [n][crop_h][crop_w][3]. */
#define VQ_RESAMPLE_BILINEAR 2      /* PIL.Image.BILINEAR */
#define VQ_RESAMPLE_BICUBIC 3       /* PIL.Image.BICUBIC */
/* cv2.resize(frame, (out_w, out_h)) with the default INTER_LINEAR — what OptimizedFrameExtractor applies
 * (frame_extractor.py:283-284): OpenCV's 11-bit two-tap bilinear without antialiasing, its exact-2x shortcut
 * to the 2x2 area average, equal sizes copied.  OpenCV is absent from the build container: restated from
 * modules/imgproc/src/resize.cpp, parity unpinned. */
#define VQ_RESAMPLE_CV_LINEAR 100
typedef struct vq_resampler vq_resampler;
int vq_resampler_create(vq_resampler** out);
int vq_resampler_destroy(vq_resampler* r);
int vq_resampler_set_stream(vq_resampler* r, void* hip_stream);
int vq_resampler_synchronize(vq_resampler* r);
/* Host frames in; host result out, or (out == NULL) left in the handle's device buffer for
 * vq_encoder_encode_u8_device.  Returns when the result is complete. */
int vq_resampler_run_u8(vq_resampler* r, const uint8_t* frames, int n, int h, int w, int filter,
                        int out_h, int out_w, int crop_top, int crop_left, int crop_h, int crop_w, uint8_t* out);
/* Same for n separately allocated frames of one size (a Python list of ndarray frames). */
int vq_resampler_run_u8_list(vq_resampler* r, const uint8_t* const* frames, int n, int h, int w, int filter,
                             int out_h, int out_w, int crop_top, int crop_left, int crop_h, int crop_w, uint8_t* out);
/* Device frames in, device result out (d_out == NULL: the handle's buffer); asynchronous on the handle's stream. */
int vq_resampler_run_u8_device(vq_resampler* r, const uint8_t* d_frames, int n, int h, int w, int filter,
                               int out_h, int out_w, int crop_top, int crop_left, int crop_h, int crop_w, uint8_t* d_out);
int vq_resampler_device_output(vq_resampler* r, void** d_ptr, int64_t* bytes);
/* Output size and crop offsets of the CLIP image processor for an h x w frame
 * (transformers image_transforms.py:295-299 get_resize_output_image_size + centre crop). */
int vq_clip_processor_geometry(int h, int w, int size, int crop, int* resized_h, int* resized_w,
                               int* crop_top, int* crop_left);
/* OptimizedFrameExtractor._is_low_quality inputs (frame_extractor.py:301-316) for BGR uint8 frames:
 * mean_brightness[i] = np.mean(frame_i); laplacian_var[i] = cv2.Laplacian(BGR2GRAY(frame_i), CV_64F).var().
 * on_device != 0: `frames` is a device pointer.  (OpenCV is absent from the build container: this
 * restates its published fixed-point grey conversion and 4-neighbour stencil; parity unpinned.) */
int vq_frame_quality_u8(vq_resampler* r, const uint8_t* frames, int n, int h, int w, int on_device,
                        double* mean_brightness, double* laplacian_var);
/* AdaptiveFrameSampler._calculate_frame_difference (frame_extractor.py:168-186) for every consecutive pair of
 * BGR uint8 frames [n][h][w][3]: score[i] compares frames[i-1] (earlier) with frames[i]; score[0] compares
 * prev_frame (ONE h x w x 3 frame of the same residency as `frames`) with frames[0], or is 0.0 when prev_frame
 * is NULL (the reference's first frame carries scene_change_score 0.0).  mse / hist_diff (optional, may be
 * NULL) receive the two terms.  on_device != 0: frames and prev_frame are device pointers of any alignment.
 * Results are host doubles; returns when they are complete.
 *   mse       = np.mean((grey_a.astype(float) - grey_b.astype(float)) ** 2): an exact integer sum, one division;
 *   hist_diff = cv2.compareHist(hist_a, hist_b, HISTCMP_CHISQR): sum over ascending bins with hist_a != 0 of
 *               (hist_a - hist_b)^2 / hist_a in fp64, the earlier frame supplying the denominators;
 *   score     = mse + hist_diff * 0.01.
 * h * w <= 2^24 (histogram counts stay exact in OpenCV's float32 bins), n <= 65535; n == 0 is a no-op.  Host
 * frames go up in slices of at most 512 MiB ($VQ_AMD_SCENE_SLICE_BYTES, read per call, overrides the budget).
 * Grey is the fixed-point BGR2GRAY restated for vq_frame_quality_u8 (parity with OpenCV unpinned, as there);
 * OpenCV does not fix the order of compareHist's sum, so its hist_diff may differ from this one in the last bits. */
int vq_frame_scene_scores_u8(vq_resampler* r, const uint8_t* frames, int n, int h, int w, int on_device,
                             const uint8_t* prev_frame, double* score, double* mse, double* hist_diff);

/* OptimizedFrameExtractor.extract_frames' per-frame work (frame_extractor.py:279-293) for a batch of BGR uint8 frames
 * [n][h][w][3] in one device pass: cv2.resize to out_w x out_h (VQ_RESAMPLE_CV_LINEAR, bit-identical to
 * vq_resampler_run_u8 with that filter), the three integer sums behind _is_low_quality taken from on-chip memory
 * while the resized frame is written, the keep / drop verdict on the device, and the survivors compacted in input order.
 *   out_h == out_w == 0: no resize (frame_size=None): the statistics are those of the frames as given.
 *   quality_filter == 0: every frame is kept; the sums are computed only when `sums` is given.
 *   keep [n]: 1 = kept.  sums [n][3] (may be NULL) = {sum of all bytes, sum L, sum L^2}, L the 4-neighbour Laplacian
 *     (BORDER_REFLECT_101) of the fixed-point BGR2GRAY image, as for vq_frame_quality_u8.
 *   A frame is dropped when, with N = out_h * out_w:  sum_bytes < 20 * 3 * N,  or  sum_bytes > 235 * 3 * N,  or
 *     N * sumL2 - sumL^2 < 100 * N^2  — mean brightness < 20 or > 235, Laplacian variance < 100, decided in exact
 *     integers.  out_h * out_w <= 2^21 keeps every term inside int64; larger outputs are VQ_ERR_INVALID.
 *   out: host memory for n frames, of which the first *n_kept are written.  out == NULL: the result stays on the
 *     device; vq_resampler_device_output returns its address, it is *n_kept frames long and valid until the next
 *     call on the handle.
 * on_device != 0: `frames` is a device pointer of any alignment.  n <= 65535; n == 0 is a no-op with *n_kept = 0.
 * All forms return when the result is complete.  Host frames go up in slices of at most 512 MiB
 * ($VQ_AMD_POSTPROC_SLICE_BYTES, read per call, overrides the budget); survivors of later slices follow those of
 * earlier ones.  (OpenCV parity unpinned, as for the resize and the quality statistics.) */
int vq_frame_postprocess_u8(vq_resampler* r, const uint8_t* frames, int n, int h, int w, int on_device,
                            int out_h, int out_w, int quality_filter,
                            uint8_t* out, int64_t* n_kept, uint8_t* keep /*[n]*/, int64_t* sums /*[n][3], may be NULL*/);
/* Same for n separately allocated host frames of one size. */
int vq_frame_postprocess_u8_list(vq_resampler* r, const uint8_t* const* frames, int n, int h, int w,
                                 int out_h, int out_w, int quality_filter,
                                 uint8_t* out, int64_t* n_kept, uint8_t* keep, int64_t* sums);
/* How the pass above splits an out_h x out_w output: rows per workgroup band, bands per frame, and whether a band
 * fits the on-chip budget (fused = 1 for every out_w <= 1024 at least).  fused = 0: the existing resize and
 * quality kernels run back to back on the device instead, one band per frame.  Pure host arithmetic: needs neither
 * vq_init nor a device. */
int vq_frame_postprocess_plan(int out_h, int out_w, int* band_rows, int* n_bands, int* fused);

/* What a Pillow resize (BILINEAR / BICUBIC) of n frames of h x w to out_h x out_w, cropped to crop_h x crop_w at (crop_top,
 * crop_left), would launch (csrc/preproc_plan.h).  The three A/B switches of the horizontal pass are arguments here, not the
 * environment: force_seg ($VQ_AMD_RSH=seg), lds_kb ($VQ_AMD_RSH_LDS_KB), spw ($VQ_AMD_RSH_SPW); 0 = unset.  tmp_align / dst_align:
 * address & 15 of the intermediate and of the output (0 for the handle's own buffers).
 * row_first, rows_needed: the source rows the horizontal pass produces; tmp_bytes: its intermediate.  hx: 1 the row-block-major
 * kernel, 0 the segment-major one; oc output columns per segment, whose widest source span is `span` pixels; pitch_dw dwords per
 * staged row, tile_pitch bytes per result-tile row, lds bytes of dynamic LDS; dword_store; spw segments per workgroup; the
 * horizontal grid; the two tables' row lengths; row_bytes = crop_w * 3; the vertical pass's access width (16, 4 or 1 bytes) and grid.
 * Pure host arithmetic: needs neither vq_init nor a device.  A row no LDS image holds returns VQ_ERR_INVALID, as the resize does. */
typedef struct vq_resample_plan {
    int64_t row_first, rows_needed, tmp_bytes, hx, oc, span, pitch_dw, tile_pitch, lds, dword_store, spw, hgrid_x, hgrid_y, hgrid_z;
    int64_t ksize_h, ksize_v, row_bytes, vvec, vgrid_x, vgrid_y, vgrid_z;
} vq_resample_plan;
int vq_debug_resample_plan(int h, int w, int filter, int out_h, int out_w, int crop_top, int crop_left, int crop_h, int crop_w, int n,
                           int tmp_align, int dst_align, int force_seg, int lds_kb, int spw, vq_resample_plan* out);
/* The small plans of the other paths, same header, same rules.  out[0]: frames per slice of n host frames of frame_bytes under
 * slice_budget bytes.  out[1..3]: frames per batch, histogram bytes and squared-difference bytes of a scene pass over m frames of
 * `tiles` tiles under scratch_budget bytes.  out[4..8]: the post-processing result layout of post_m frames of post_bands bands:
 * byte offsets of partials, res, prefix, keep, and the total. */
int vq_debug_preproc_small_plans(int n, int64_t frame_bytes, int64_t slice_budget, int m, int tiles, int64_t scratch_budget,
                                 int post_m, int post_bands, int64_t* out /*[9]*/);

#ifdef __cplusplus
}
#endif
#endif /* VQ_AMD_H */
