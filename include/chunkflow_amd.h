/* chunkflow_amd C-ABI — the MI355X (gfx950) hot-path extension beneath the
 * `chunkflow inference` operator surface.
 *
 * Each entry point replaces a reference hot-path function (SURVEY.md §8a/§8b;
 * reference = seung-lab/chunkflow v1.1.7):
 *   cfx_make_patch_mask      <- patch/patch_mask.py:15-68  (host, f64 internally)
 *   cfx_cast_u8_f32_div      <- inferencer.py:395-399      (int chunk -> f32 / dtype_max)
 *   cfx_normalize_intensity  <- flow/flow.py:1650-1669     (u8 -> f32, x/127.5 - 1)
 *   cfx_extract_patches      <- inferencer.py:408-411 + chunk/base.py:761-781
 *   cfx_blend_accumulate     <- inferencer.py:436-455 + chunk/base.py:792-807
 *                               (fuses the engine's patch-mask multiply,
 *                                pytorch.py:113, when mask != NULL)
 *   cfx_build_chunk_mask     <- inferencer.py:294-333
 *   cfx_reciprocal           <- inferencer.py:333
 *   cfx_multiply_mask        <- inferencer.py:460-461 (ufunc chunk/base.py:418-453)
 *   cfx_max                  <- inferencer.py:463-466 (assert < 1.0001)
 *   cfx_crop_margin          <- chunk/base.py:691-726 (flow.py:2053-2084)
 *   cfx_mask_using_last_channel <- chunk/base.py:685-689 (inferencer.py:468-477)
 *   cfx_gaussian2d           <- chunk/base.py:846-853 (flow.py:1615-1630)
 *   cfx_median3d             <- plugins/median_filter.py
 *
 * Conventions: the caller owns every buffer (device pointers come from
 * torch-ROCm tensors' data_ptr()); layout is contiguous C-order z-y-x with x
 * fastest; all calls are stream-ordered on the context stream (adopt torch's
 * stream via cfx_set_stream); int return = 0 on success, nonzero with
 * cfx_last_error() set; one context per GPU rank, single-threaded per
 * context.
 */
#ifndef CHUNKFLOW_AMD_H
#define CHUNKFLOW_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cfx_ctx cfx_ctx;

/* ---- lifecycle -------------------------------------------------------- */
cfx_ctx* cfx_init(int device);
void     cfx_destroy(cfx_ctx* ctx);
const char* cfx_last_error(void);
int      cfx_version(void);
/* adopt an existing HIP stream (e.g. torch.cuda.current_stream().cuda_stream);
 * stream may be NULL for the legacy default stream */
int cfx_set_stream(cfx_ctx* ctx, void* hip_stream);
int cfx_sync(cfx_ctx* ctx);

/* ---- host precompute --------------------------------------------------- */
/* Wu bump-weight patch mask, float64 pipeline, f32 result (pz*py*px floats).
 * Runs on the HOST; upload the result once per geometry. */
int cfx_make_patch_mask(const int patch_size[3], const int overlap[3],
                        float* out);

/* ---- device kernels (all pointers are DEVICE pointers) ----------------- */
/* Alignment contract: any element-aligned pointer is accepted. The float4
 * (uchar4) fast paths of cfx_normalize_intensity / cfx_cast_u8_f32_div,
 * cfx_extract_patches, cfx_blend_accumulate, cfx_blend_batch,
 * cfx_multiply_mask(_max) and cfx_crop_margin are taken only when, besides
 * the size and offset conditions, every f32 base pointer of the call is
 * 16-byte aligned (the u8 source: 4-byte aligned); otherwise the scalar
 * path computes the same bits. Allocations are always aligned; a view that
 * starts at an odd element of one is not. */
/* out[i] = (float)in[i] / 127.5f - 1.0f */
int cfx_normalize_intensity(cfx_ctx* ctx, const unsigned char* in, float* out,
                            long long n);
/* out[i] = (float)in[i] / divisor  (divisor = integer dtype max) */
int cfx_cast_u8_f32_div(cfx_ctx* ctx, const unsigned char* in, float* out,
                        long long n, float divisor);
/* gather n_patches windows of an f32 chunk (channels, D, H, W) into a batch
 * buffer (n_patches, channels, pz, py, px); starts_zyx is a HOST array of
 * n_patches*3 ints, chunk-local coordinates */
int cfx_extract_patches(cfx_ctx* ctx, const float* chunk, int channels,
                        const int chunk_dims[3], const int* starts_zyx,
                        int n_patches, const int patch_size[3], float* out);
/* out[c, region] += patch[c, region'] * mask[region'], clipped to the output
 * bounds; offset_zyx is the patch start relative to the output buffer origin;
 * mask may be NULL (plain accumulate, e.g. a pre-masked universal plugin) */
int cfx_blend_accumulate(cfx_ctx* ctx, float* out, int channels,
                         const int out_dims[3], const float* patch,
                         const int patch_dims[3], const int offset_zyx[3],
                         const float* mask);
/* many-patch blend in ONE launch: items is a HOST array of n*4 ints
 * (batch_index, oz, oy, ox). The caller must guarantee the clipped output
 * regions are pairwise DISJOINT (see the first-fit grouping in
 * chunkflow_amd/grouping.py) so the accumulate stays atomics-free and
 * bit-ordered; >32 items are split across launches. */
int cfx_blend_batch(cfx_ctx* ctx, float* out, int channels,
                    const int out_dims[3], const float* patch,
                    const int patch_dims[3], const int* items, int n,
                    const float* mask);
/* zero mask_out (out_dims), blend patch_mask at each of n offsets (HOST
 * array, n*3 ints, relative to the output origin), then reciprocal */
int cfx_build_chunk_mask(cfx_ctx* ctx, float* mask_out, const int out_dims[3],
                         const float* patch_mask, const int patch_dims[3],
                         const int* offsets_zyx, int n);
int cfx_reciprocal(cfx_ctx* ctx, float* buf, long long n);
/* out[c*n + i] *= mask[i] for every channel c (mask-normalize) */
int cfx_multiply_mask(cfx_ctx* ctx, float* out, const float* mask,
                      int channels, long long n_voxels);
/* synchronous max over n floats (the <1.0001 sanity assert). If the buffer
 * holds a NaN of either sign at any position, *host_max is NaN, so that
 * `max < 1.0001` fails as the reference's assert_array_less does; otherwise
 * it is the largest element. */
int cfx_max(cfx_ctx* ctx, const float* buf, long long n, float* host_max);
/* fused mask-normalize + max scan (saves a full output read pass);
 * returns -2 when n_voxels is not a multiple of 4 or out / mask is not
 * 16-byte aligned — multiply done, call cfx_max yourself. *host_max is the
 * max of the PRODUCT and, like cfx_max, NaN whenever the product holds a
 * NaN of either sign; the multiply itself is not affected. */
int cfx_multiply_mask_max(cfx_ctx* ctx, float* out, const float* mask,
                          int channels, long long n_voxels,
                          float* host_max);
/* contiguous copy dropping margins[6] = -z,-y,-x,+z,+y,+x */
int cfx_crop_margin(cfx_ctx* ctx, const float* in, float* out, int channels,
                    const int in_dims[3], const int margins[6]);
/* out[(channels-1), dims] = in[:channels-1] * (in[channels-1] < threshold) */
int cfx_mask_using_last_channel(cfx_ctx* ctx, const float* in, float* out,
                                int channels, const int dims[3],
                                float threshold);

/* ---- connected components (cc3d replacement; config-4 chain) ----------- */
/* fg[i] = in[i] > threshold */
int cfx_threshold(cfx_ctx* ctx, const float* in, unsigned char* fg,
                  long long n, float threshold);
/* fg[i] = in[i] != 0 */
int cfx_nonzero_u8(cfx_ctx* ctx, const unsigned char* in, unsigned char* fg,
                   long long n);
/* 6/18/26-connectivity union-find labeling of a u8 foreground mask.
 * labels (u32, caller-owned) doubles as the union-find parent array;
 * scratch is a second u32 buffer of the same length. Labels are 1..N in
 * raster-scan first-encounter order (scipy.ndimage.label-compatible);
 * background is 0. */
int cfx_connected_components(cfx_ctx* ctx, const unsigned char* fg,
                             const int dims[3], int connectivity,
                             unsigned int* labels, unsigned int* scratch,
                             long long* n_components);
/* The same union-find over a label volume (elem_bytes 1, 4 or 8): a voxel
 * is foreground iff non-zero, and two neighbours are united iff their
 * values are equal as raw bit patterns (cc3d's multi-label semantics), so
 * touching regions of different value stay apart. Same numbering, limits
 * and buffers as above; seg must not alias labels or scratch. On a binary
 * volume the two entries agree. */
int cfx_connected_components_labels(cfx_ctx* ctx, const void* seg,
                                    int elem_bytes, const int dims[3],
                                    int connectivity, unsigned int* labels,
                                    unsigned int* scratch,
                                    long long* n_components);

/* ---- per-label voxel counts and label masking (mask-out-objects) -------- */
/* A label table is two caller-owned device arrays: keys u64[capacity]
 * (32-bit labels zero-extended; all-ones marks an empty slot, so the label
 * 2^64-1 is out of contract and reported as an error) and vals
 * u32[capacity] (a voxel count or a keep flag). capacity must be a power
 * of two and at least the number of distinct keys inserted; size it from
 * cfx_label_run_starts. A table that turns out too small makes the call
 * return an error ("label table full"); it never hangs. Volumes are (D, H,
 * W) of 4- or 8-byte labels compared as raw bit patterns, at most 2^32-1
 * voxels. */
/* number of voxels that differ from their flat (z,y,x-order) predecessor,
 * plus one for voxel 0: an upper bound on the number of distinct labels.
 * Synchronous. */
int cfx_label_run_starts(cfx_ctx* ctx, const void* labels, int elem_bytes,
                         const int dims[3], long long* n_runs);
/* every slot empty, every value 0 */
int cfx_label_table_clear(cfx_ctx* ctx, unsigned long long* keys,
                          unsigned int* vals, long long capacity);
/* vals[slot(id)] = value for each of n_ids device-resident u64 ids
 * (duplicates allowed). Synchronous (reads the status flags back). */
int cfx_label_table_insert(cfx_ctx* ctx, const unsigned long long* ids,
                           long long n_ids, unsigned int value,
                           unsigned long long* keys, unsigned int* vals,
                           long long capacity);
/* vals[slot(label)] += voxel count of that label, zero included, on a
 * cleared table. Synchronous (reads the status flags back). */
int cfx_label_count(cfx_ctx* ctx, const void* labels, int elem_bytes,
                    const int dims[3], unsigned long long* keys,
                    unsigned int* vals, long long capacity);
/* The contingency table of two (D, H, W) volumes of equal shape, each of 4-
 * or 8-byte labels (all four combinations): for every pair (s, g) that
 * occurs at some voxel, vals[slot(key)] += the number of such voxels, on a
 * cleared table. seg_keys / gt_keys are the key arrays of the tables that
 * cfx_label_count filled from the same two volumes (their values are not
 * read); the key of a pair is (slot of s in seg_keys << 32) | slot of g in
 * gt_keys, so single tables above 2^31 slots are refused and a pair key
 * never equals the empty marker. Counts are exact; zero is an ordinary
 * label. The number of distinct pairs is at most run_starts(seg) +
 * run_starts(gt) - 1: size the pair table from that. Errors: "label table
 * full", the reserved label 2^64-1, a label that its single table does not
 * hold, volumes that differ in shape. Synchronous (reads the status flags
 * back). */
int cfx_label_pair_count(cfx_ctx* ctx, const void* seg, int seg_bytes,
                         const int seg_dims[3],
                         const unsigned long long* seg_keys,
                         long long seg_capacity, const void* gt, int gt_bytes,
                         const int gt_dims[3],
                         const unsigned long long* gt_keys,
                         long long gt_capacity, unsigned long long* keys,
                         unsigned int* vals, long long capacity);
/* out[i] = keep(in[i]) ? in[i] : 0, zero staying zero. mode 0: keep iff the
 * label's value in the table is > threshold (dust removal over a counted
 * table); mode 1: keep iff the label is in the table with a non-zero value
 * (threshold unused). Labels absent from the table are zeroed. in == out is
 * allowed. */
int cfx_label_mask(cfx_ctx* ctx, const void* in, void* out, int elem_bytes,
                   const int dims[3], const unsigned long long* keys,
                   const unsigned int* vals, long long capacity, int mode,
                   long long threshold);

/* ---- affinity maps to segments (watershed + region graph) -------------- */
/* aff is f32 (3, D, H, W), contiguous, channels x, y, z: aff[c][v] is the
 * weight of the edge between voxel v and its predecessor along that axis
 * (the leading face of each axis belongs to no edge and is never read).
 * All compares are f32; NaN fails every test. */
/* Watershed fragments, a steepest-ascent forest: an edge is live iff
 * w >= low and strong iff live and w >= high; a voxel with a live incident
 * edge picks the first one in the order -x +x -y +y -z +z whose weight is
 * the maximum over its live incident edges; fragments are the connected
 * components under the strong and the picked edges, numbered 1..N by first
 * voxel in raster order; a voxel without a live incident edge is 0. With
 * low == high == T these are the components of the edges >= T. labels and
 * scratch are u32 buffers of D*H*W elements (fewer than 2^32-1), as for
 * cfx_connected_components. Synchronous. */
int cfx_affinity_fragments(cfx_ctx* ctx, const float* aff, const int dims[3],
                           float low, float high, unsigned int* labels,
                           unsigned int* scratch, long long* n_components);
/* The region graph of a u32 fragment volume: one row per pair a < b of
 * different non-zero ids joined by at least one edge, keyed (a << 32) | b in
 * a table of the kind above with a second value array: counts[slot] is the
 * number of such edges, sums[slot] the sum of q(w) over them, q(w) =
 * floor(c * 2^24) with c = w > 0 ? min(w, 1) : 0 (NaN and negative weights
 * give 0), so a row's mean affinity is sums / (counts * 2^24) and the rows
 * are bit-exact whatever the order of the adds. The call clears the table
 * first. capacity is a power of two and at least the number of rows: size
 * it from cfx_region_graph_runs, which returns the number of table
 * operations the call makes (one per run of equal pairs within a lane's
 * stretch of a row), an upper bound on the rows. At most (2^32-1)/3
 * voxels. Errors: "label table full". Both synchronous. */
int cfx_region_graph_runs(cfx_ctx* ctx, const unsigned int* frag,
                          const int dims[3], long long* n_runs);
int cfx_region_graph(cfx_ctx* ctx, const unsigned int* frag,
                     const float* aff, const int dims[3],
                     unsigned long long* keys, unsigned int* counts,
                     unsigned long long* sums, long long capacity);

/* ---- image normalization (normalize-contrast operator) ----------------- */
/* zero + accumulate nsec 256-bin u32 histograms, one per contiguous
 * n_per_sec-voxel section of a u8 volume */
int cfx_hist_u8(cfx_ctx* ctx, const unsigned char* in, long long n_per_sec,
                int nsec, unsigned int* hist);
/* in-place per-section LUT gather: buf[i] = lut[sec][buf[i]] */
int cfx_lut_apply_u8(cfx_ctx* ctx, unsigned char* buf, long long n_per_sec,
                     int nsec, const unsigned char* lut);

/* ---- image filters (gaussian-filter operator, median_filter plugin) ----- */
/* Per-section 2-D gaussian of `sections` contiguous (height, width) images,
 * uint8 or float32 (is_f32), bit-pinned to scipy.ndimage.gaussian_filter:
 * the y pass, then the x pass, each t = v[i]*w[r], then for k = -r..-1
 * t += (v[i+k] + v[i-k]) * w[k+r] in f64 with nothing fused, 'reflect'
 * borders (d c b a | a b c d | d c b a, any radius against any length), and
 * the result of EACH pass converted to the volume's dtype (f32 rounds to
 * nearest, u8 truncates). wy / wx are DEVICE arrays of 2*r+1 normalised f64
 * weights that the caller computes; the library never recomputes them. A
 * NULL weight pointer with radius 0 skips that axis. Radii above 24 (the
 * halo an LDS tile holds) are an error, never a wrong answer. in != out.
 * Not timed into any profile slot. */
int cfx_gaussian2d(cfx_ctx* ctx, const void* in, void* out, int is_f32,
                   long long sections, int height, int width,
                   const double* wy, int ry, const double* wx, int rx);
/* 3-D median of `volumes` contiguous (D, H, W) volumes, uint8 or float32:
 * the element of rank N/2 of the N = size[0]*size[1]*size[2] values of the
 * window centred on each voxel, as scipy.ndimage.median_filter gives it.
 * Every size entry is odd, N <= 125. mode: 0 reflect, 1 nearest, 2 mirror,
 * 3 constant (value 0), 4 wrap, each with scipy's meaning. Float NaN and
 * the sign of zero are out of contract. in != out. Not timed into any
 * profile slot. */
int cfx_median3d(cfx_ctx* ctx, const void* in, void* out, int is_f32,
                 long long volumes, const int dims[3], const int size[3],
                 int mode);

/* ---- downsample (mip pyramid; the reference's downsample operator) ------ */
/* Box average of a (channels, D, H, W) volume by factor[3] (z,y,x, any
 * positive ints); out is (channels, ceil(D/fz), ceil(H/fy), ceil(W/fx)).
 * Edge cells average the voxels that exist. Bit-pinned to the reference's
 * lib/igneous/downsample.py: f32 sum from 0 with x-offset slowest and
 * z-offset fastest, f64 quotient sum/count, then round-to-nearest (f32) or
 * truncation (u8). Factors in {1,2} on 16-byte-aligned rows take a vector
 * path. */
int cfx_downsample_avg_u8(cfx_ctx* ctx, const unsigned char* in,
                          unsigned char* out, int channels,
                          const int in_dims[3], const int factor[3]);
int cfx_downsample_avg_f32(cfx_ctx* ctx, const float* in, float* out,
                           int channels, const int in_dims[3],
                           const int factor[3]);
/* COUNTLESS 2D mode pooling of a (D, H, W) label volume: 2x2 over the two
 * axes other than preserved_axis (0=z, 1=y, 2=x). elem_bytes is 4 or 8;
 * labels compare as raw bit patterns. A pooled axis of odd length n is
 * front-mirrored ([v0,v0,v1,..]), so its output length is (n+1)/2. */
int cfx_downsample_mode2(cfx_ctx* ctx, const void* in, void* out,
                         int elem_bytes, const int in_dims[3],
                         int preserved_axis);
/* COUNTLESS 3D mode pooling, 2x2x2; every dimension must be even */
int cfx_downsample_mode3(cfx_ctx* ctx, const void* in, void* out,
                         int elem_bytes, const int in_dims[3]);

/* ---- hand-written MFMA convolution (RSUNet ResBlock 3x3x3) -------------- */
/* NDHWC f32, stride 1, pad 1, C == K in {28, 36, 48, 64}; wgt layout
 * (27, C, K) with tap = ((dz+1)*3 + (dy+1))*3 + (dx+1); bias may be NULL;
 * residual (same layout as out) may be NULL; do_elu applies ELU(alpha=1)
 * after bias/residual. profile bytes field carries FLOPs for this id. */
int cfx_conv3_ndhwc(cfx_ctx* ctx, const float* in, const float* wgt,
                    const float* bias, const float* residual, float* out,
                    int N, int D, int H, int W, int C, int K, int do_elu);
/* the persistent-z ring variant (weights LDS-resident, one input plane
 * staged per z; C == K == 28 instantiated) */
int cfx_conv3_ndhwc_zring(cfx_ctx* ctx, const float* in, const float* wgt,
                          const float* bias, const float* residual,
                          float* out, int N, int D, int H, int W, int C,
                          int K, int do_elu);
/* bf16 persistent-z ring (v_mfma_f32_32x32x16_bf16; C == K in
 * {28, 36, 48}): in/out/residual are bf16 NDHWC, wgt is a bf16 zero-padded
 * [tap][j][c] pack — (27, 32, 32) for C == 28, (27, 64, 48) for 36/48
 * (those run as four c-half x j-tile launches; partial sums round through
 * bf16 between the halves) — bias stays f32; epilogue math in f32 */
int cfx_conv3_ndhwc_bf16(cfx_ctx* ctx, const void* in, const void* wgt,
                         const float* bias, const void* residual,
                         void* out, int N, int D, int H, int W, int C,
                         int K, int do_elu);

/* ---- up/down-sampling convs (RSUNet (1,2,2)-kernel, (1,2,2)-stride) ----- */
/* ConvTranspose3d: out (N,D,2H,2W,K) from in (N,D,H,W,C), NDHWC; wgt
 * packed [parity q=(py<<1)|px][C][K] in the compute dtype; bias f32 or
 * NULL; is_bf16 selects bf16 vs f32 tensors. HBM-streaming kernels: f32
 * shapes with C % 4 == 0, K % 4 == 0, K <= 48 run on the f32 MFMA, the
 * rest (and bf16) on the VALU kernel. */
int cfx_upconv_2x2(cfx_ctx* ctx, const void* in, const void* wgt,
                   const float* bias, void* out, int N, int D, int H,
                   int W, int C, int K, int is_bf16);
/* the same transposed conv with the decoder's skip-add in its epilogue:
 * out = (bias + sum_c in * w) + skip, skip an f32 NDHWC tensor of out's
 * shape; the add is the last f32 operation, so the result equals
 * cfx_upconv_2x2 followed by a separate add bit for bit. skip == NULL is
 * cfx_upconv_2x2. With skip: f32 only (is_bf16 is an error), C % 4 == 0,
 * K % 4 == 0, C <= 64, K <= 48, in/skip/out 16-byte aligned -- the shapes
 * of the f32 MFMA kernel, which cfx_upconv_2x2 also takes for them */
int cfx_upconv_2x2_add(cfx_ctx* ctx, const void* in, const void* wgt,
                       const float* bias, const void* skip, void* out,
                       int N, int D, int H, int W, int C, int K,
                       int is_bf16);
/* one-pass epilogue behind a bias-free MIOpen conv: in place on the NDHWC
 * f32 tensor y (nvox positions x K channels),
 * y = act(y + bias[k] (+ res)), act = ELU(alpha=1) if do_elu; bias and
 * res (y's layout) may be NULL. Not timed into any profile slot. */
int cfx_bias_res_elu(cfx_ctx* ctx, float* y, const float* bias,
                     const float* res, long long nvox, int K, int do_elu);
/* strided Conv3d (downsample): out (N,D,H/2,W/2,K) from in (N,D,H,W,C);
 * same wgt pack/convention as cfx_upconv_2x2 */
int cfx_downconv_2x2(cfx_ctx* ctx, const void* in, const void* wgt,
                     const float* bias, void* out, int N, int D, int H,
                     int W, int C, int K, int is_bf16);
/* single-channel (1,5,5) conv, pad (0,2,2) — RSUNet conv_in; in
 * (N,D,H,W,1), out (N,D,H,W,K) NDHWC; wgt [K][25] row-major (dy*5+dx) in
 * the compute dtype; K <= 32 */
int cfx_conv155_c1(cfx_ctx* ctx, const void* in, const void* wgt,
                   const float* bias, void* out, int N, int D, int H,
                   int W, int K, int is_bf16);
/* few-output-channel (1,5,5) conv, pad (0,2,2) — RSUNet conv_out; in
 * (N,D,H,W,C), out (N,D,H,W,K) NDHWC, any N, D, H, W >= 1 with
 * N*D <= 65535; C == 28, K == 3 instantiated. wfrag is always f32 (for
 * bf16 the values are pre-rounded to bf16), packed as the 35 MFMA B
 * fragments [dy*7 + c/4][lane = (c%4)*16 + j], j = dx*3 + k, column
 * j == 15 zero: 35*64 floats */
int cfx_conv155_out(cfx_ctx* ctx, const void* in, const float* wfrag,
                    const float* bias, void* out, int N, int D, int H,
                    int W, int C, int K, int is_bf16);
/* the 32x32x2-MFMA variant (C == K == 28 instantiated) */
int cfx_conv3_ndhwc_w32(cfx_ctx* ctx, const float* in, const float* wgt,
                        const float* bias, const float* residual,
                        float* out, int N, int D, int H, int W, int C,
                        int K, int do_elu);

/* ---- kernel timing (HIP events on the context stream) ------------------ */
enum cfx_kernel_id {
    CFX_K_BLEND = 0,
    CFX_K_EXTRACT = 1,
    CFX_K_NORMALIZE = 2,
    CFX_K_CAST = 3,
    CFX_K_RECIPROCAL = 4,
    CFX_K_MASKMUL = 5,
    CFX_K_CROP = 6,
    CFX_K_MAX = 7,
    CFX_K_MYELIN = 8,
    CFX_K_CC = 9,
    CFX_K_CONV = 10,
    CFX_K_CONV_STREAM = 11,  /* up/down-sample + (1,5,5) stream convs */
    CFX_K_LABELS = 12,       /* label run-start / count / pair / mask passes */
    CFX_K_COUNT = 13
};
int cfx_profile_enable(cfx_ctx* ctx, int enable);
int cfx_profile_reset(cfx_ctx* ctx);
/* drains pending events (syncs the stream); bytes = accumulated ALGORITHMIC
 * bytes of the profiled launches (computed from region sizes, not counters) */
int cfx_profile_get(cfx_ctx* ctx, int kernel_id, unsigned long long* count,
                    double* total_ms, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* CHUNKFLOW_AMD_H */
