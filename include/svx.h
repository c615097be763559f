/* svx.h -- C ABI of libsvx.so, the MI355X (gfx950) hot path of SVision.
 *
 * The reference (xjtu-omics/SVision v1.4) is pure Python and has no FFI layer;
 * each entry point below replaces one Python hot loop and is bound from the
 * Python host with ctypes (svision_amd/_lib.py; INTEGRATION.md shows the stub a
 * reference maintainer would add).  Conventions:
 *   - every pointer named d_* is a DEVICE pointer owned by the caller
 *     (e.g. a torch tensor's data_ptr()); nothing is allocated or freed inside;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all
 *     work is enqueued asynchronously on it, no host synchronisation inside;
 *   - return value: 0 on success, a negative SVX_E* code otherwise; never throws;
 *   - re-entrant; one process per GPU.
 */
#ifndef SVX_H
#define SVX_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVX_VERSION 420            /* 0.3.0: + svx_bgzf_crc32, svx_bgzf_inflate_fast (360); + svx_bgzf_inflate_fast_on: the two kernels on two streams (370);
                                    * svx_bgzf_inflate_fast / _on take the inflated byte count and refuse a workspace that is too small (380);
                                    * + svx_cigar_scan_flat: the scan of long alignments in one pass (390); svx_cigar_scan takes the word count of its launch, its workspace's size and shape flags (400);
                                    * the exports the default path never calls moved to svx_experimental.h, + svx_bgzf_inflate_fast_lz there (410);
                                    * svx_bam_walk_extract takes the number of records (a wave per record copies: ONT-shaped slices 14.7 -> ~1 ms) (420);
                                    * svx_bgzf_inflate_fast / _on resolve the LZ copies in a table in LDS where the device has room for it, svx_bgzf_inflate_fast_lz takes lz_kernel 3 (420, additive:
                                    * no signature changed) */

#define SVX_OK            0
#define SVX_EINVAL       (-1)      /* bad argument (null pointer, bad layout...) */
#define SVX_ECAPACITY    (-2)      /* caller-provided output capacity too small */
#define SVX_ELAUNCH      (-3)      /* HIP reported a launch error */

#define SVX_IMG           227      /* similarity image is 227 x 227 x 3 */
#define SVX_LAYOUT_NHWC   0        /* [n][227][227][3]  (reference batch layout) */
#define SVX_LAYOUT_NCHW   1        /* [n][3][227][227]  (planar, for the CNN)    */

#define SVX_GAP_INS       1
#define SVX_GAP_DEL       2

#define SVX_CONV_DENSE_PCT 97      /* a pixel list this full (percent) is not followed: svx_conv2d_same computes every pixel */

/* "C8" activation layout of the CNN entry points: float32 [image][C/8][H][W][8] -- channel c of pixel (y, x) lives at
 * ((image * C/8 + c/8) * H*W + y*W + x) * 8 + c%8, so the 8 channels of an octet are one 32-byte sector per pixel
 * (C % 8 == 0).  It lets every MFMA operand fetch and every epilogue store of svx_conv2d_same be a 16-byte access of
 * whole sectors, for dense pixel ranges and for gathered (active-set) pixels alike. */

/* One long CIGAR gap (I or D with length >= min_sv), 24 bytes.
 * Replaces the entries of `all_long_gaps` built at
 * reference src/collection/analyze_reads.py:828-853. */
typedef struct SvxGap {
    uint32_t aln;        /* alignment index in the batch                       */
    uint32_t op;         /* index of the op inside that alignment's CIGAR      */
    int32_t  read_pos;   /* readPos before the op (leading clips included)     */
    int32_t  ref_pos;    /* refPos before the op                               */
    int32_t  len;        /* op length                                          */
    uint32_t kind;       /* SVX_GAP_INS / SVX_GAP_DEL                          */
} SvxGap;

int         svx_version(void);
const char* svx_strerror(int code);
/* host: crc32c (Castagnoli) of a buffer -- the tensor / block checksums of the -m checkpoint (predict.py:181-184's
 * Saver().restore verifies them inside TensorFlow) */
uint32_t    svx_crc32c(const void* data, size_t n);

#define SVX_SCAN_FAILED   0xFFFFFFFFu

/* Bytes of device scratch svx_cigar_scan needs for n_aln alignments of n_words CIGAR words (the frame records of its long
 * alignments and the map of their launch take n_words * 5 / 128 bytes of it). */
size_t svx_cigar_scan_ws_bytes(uint32_t n_aln, uint64_t n_words);

/* flags of svx_cigar_scan: 0 = the count pass's shape follows the launch's mean words per alignment; the bits fix it (A/B runs,
 * tests) -- never a result */
#define SVX_SCAN_LANES4   1u       /* four lanes per alignment (default up to 256 words per alignment) */
#define SVX_SCAN_LANES8   2u       /* eight */
#define SVX_SCAN_SHARED   4u       /* the frames of long alignments in a launch of their own, equal ranges of the array (default from 1,024 words per alignment) */
#define SVX_SCAN_UNSHARED 8u       /* a long alignment is finished by its own wave */

/* Per-alignment CIGAR / segment scan.
 * Replaces the Python loop of analyze_inside_align
 * (reference src/collection/analyze_reads.py:828-853) and the pysam-derived
 * reference_end / query_alignment_start / query_alignment_end
 * (src/collection/analyze_reads.py:650-667) for a whole batch of alignments.
 *
 *   d_cigar     packed BAM CIGAR words (len << 4 | op) of all alignments, concatenated;
 *               16-byte aligned (read in quads), d_cig_off[n_aln] words long
 *   d_cig_off   [n_aln + 1] word offsets into d_cigar (CSR)
 *   d_ref_start [n_aln] 0-based reference start of each alignment
 *   min_sv      options.min_sv_size
 *   d_gaps      [gaps_cap] out: long gaps sorted by (aln, op)
 *   d_gap_off   [n_aln + 1] out, 16-byte aligned: CSR offsets into d_gaps per alignment
 *               (d_gap_off[n_aln] = total number of long gaps, even when it
 *               exceeds gaps_cap; gaps beyond gaps_cap are not written;
 *               SVX_SCAN_FAILED = the offsets pass gave up waiting for a tile in front of it
 *               -- workgroups are dispatched in index order on this hardware, so this is a
 *               bug or a different dispatcher, never data --: the other outputs are invalid)
 *   d_stats     [n_aln][4] out, may be NULL: ref_span (M,D,N,=,X),
 *               lead_clip (leading S/H), trail_clip (trailing S/H),
 *               query_len (M,I,S,H,=,X)
 *   d_ws        scratch of ws_bytes >= svx_cigar_scan_ws_bytes(n_aln, n_words) bytes, 16-byte aligned, contents ignored
 *   n_aln       < 2^30
 *   n_words     the CIGAR words d_cigar holds, >= d_cig_off[n_aln] (the caller knows it as the length of its array; an array that
 *               holds more than it said: SVX_SCAN_FAILED in d_gap_off[n_aln]).  It sizes the frame records and picks the count pass's shape
 * Three launches (count -> offsets, its prefix over the tiles by a decoupled look-back -> emit), no atomics on results.
 * An alignment of more than 512 words (1,024 in launches of 257-1,024 words per alignment) is cut, behind that head, into frames
 * of 512 words whose sums the count pass keeps: the emit pass walks only the frames that hold a long gap.  A launch of long alignments (more than 1,024 words each on average: ONT, contigs)
 * takes the frames in a launch of its own between count and offsets, the array cut into equal ranges.
 * H is treated as S (the reference rewrites H to S, collect_signatures.py:91);
 * N advances the read position only (analyze_reads.py:831-832). */
int svx_cigar_scan(const uint32_t* d_cigar, const uint64_t* d_cig_off,
                   const int32_t* d_ref_start, uint32_t n_aln, uint64_t n_words, int32_t min_sv,
                   SvxGap* d_gaps, uint64_t gaps_cap, uint32_t* d_gap_off,
                   int32_t* d_stats, void* d_ws, uint64_t ws_bytes, uint32_t flags, void* stream);

/* Similarity-image rasteriser (+ mean subtraction, + layout).
 * Replaces BatchGenerator.next_batch's per-image loop
 * (reference src/network/create_batch.py:103-152) and PlotSingleImg.plot
 * (src/segmentplot/plot_segment.py:33-68, incl. cv2.line) for n images.
 *
 *   d_records  [n][12] int32: seg1 x_start,x_end,y_start,y_end,forward(0/1),
 *              seg2 idem, read_len, ref_len  (TSV columns 1..12)
 *   d_out      float32 [n][227][227][3] (NHWC) or [n][3][227][227] (NCHW):
 *              255 - mean[c] on line pixels, -mean[c] elsewhere
 *   mean       host pointer to 3 floats (reference: 104, 117, 124) */
int svx_rasterize(const int32_t* d_records, uint32_t n, float* d_out, int layout,
                  const float* mean, void* stream);

/* Encode + first CNN layer without materialising the image ("sparse conv1").
 * Replaces, for n segment pairs, BatchGenerator.next_batch + PlotSingleImg.plot (as svx_rasterize)
 * AND conv1 -> relu -> pool1 -> norm1 of the reference graph (src/network/alexnet.py:29-31):
 * the image is 255 on a few hundred line pixels and 0 elsewhere, so the 11x11/4 VALID convolution
 * of the mean-subtracted image is base[k] + 255 * (sum of the weight rows of the set pixels).
 *   d_records [n][12] int32 as for svx_rasterize
 *   d_w1      conv1/weights in checkpoint layout HWIO [11][11][3][96], 16-B aligned
 *   d_base    [96]: biases[k] - sum_{ky,kx,ch} mean[ch] * w[ky][kx][ch][k], 16-B aligned
 *   d_y       float32 [n][12][27][27][8] (C8) = norm1 output
 *   d_touched [n][27] or NULL: bit x of word [i][y] = pooled pixel (y, x) of image i has a set tap under it; every
 *             other pixel holds the same constant vector (the response to an empty image) */
int svx_encode_conv1(const int32_t* d_records, uint32_t n, const float* d_w1, const float* d_base, float* d_y,
                     int lrn, uint32_t radius, float alpha, float beta, float k, uint32_t* d_touched, void* stream);

/* Active sets of the AlexNet body (conv2 5x5 on 27x27 -> pool 3x3/2 -> conv3..conv5 3x3 on 13x13,
 * src/network/alexnet.py:34-46): the outputs that can differ from the network's response to an empty image, given
 * the touched pixels of the first layer.  The similarity image is a few thin lines, so only ~37 % of conv2's and
 * 50-90 % of conv3..5's outputs have a line in their receptive field; all others equal a precomputed, image
 * independent background tensor (exactly: every operation is local).
 *   d_list2 [n*729], d_list3 / d_list4 / d_list5 [n*169]: out, permutations of all pixel ids image * H*W + y * W + x:
 *             the active ones first (ascending), then the inactive ones (ascending)
 *   d_counts [4]: out, number of active entries in the four lists;  d_ws: scratch, 16 * n bytes, 16-B aligned
 *   d_totals: NULL, or uint64 [5] running sums the launch ADDS to (never cleared here): [0..4) the output pixels
 *             svx_conv2d_same computes for conv2..conv5 given these lists (all of them once a list is
 *             SVX_CONV_DENSE_PCT full), [4] images -- the executed work of a run, for measurement
 *   d_active2: NULL, or out [n][27]: bit x of word [i][y] = conv2 output pixel (y, x) of image i is in the active set
 *             (what svx_bias_relu_pool_lrn needs to read the others from the background tensor) */
int svx_alexnet_active_sets(const uint32_t* d_touched, uint32_t n, int32_t* d_list2, int32_t* d_list3,
                            int32_t* d_list4, int32_t* d_list5, uint32_t* d_counts, uint32_t* d_ws,
                            uint64_t* d_totals, uint32_t* d_active2, void* stream);

/* Fused conv epilogue: bias add + ReLU + 3x3/2 VALID max-pool (+ TF local response
 * normalisation across channels when lrn != 0), C8 float32 in and out.
 * Replaces the elementwise chain between two convolutions of the reference graph:
 * tf.nn.bias_add + relu (src/network/alexnet.py:132-135), max_pool (:158-161), lrn (:164-166)
 * as composed at alexnet.py:29-31, :34-36, :45-46.
 *   d_x   C8 [n][channels/8][height][width][8]  raw convolution output (no bias); channels % 8 == 0
 *   d_y   C8 [n][channels/8][(height-3)/2+1][(width-3)/2+1][8]          (d_x, d_bias, d_y 16-byte aligned)
 *   LRN:  y = p / (k + alpha * sum_{|j-c| <= radius} p_j^2)^beta   (alpha NOT divided by the window)
 *   d_active_rows + d_background: both NULL, or [n][height] row masks (bit x = pixel (y, x) of d_x was computed; width <= 32)
 *         and the C8 [channels/8][height][width][8] raw response of the producing convolution to an empty image: pixels
 *         whose bit is clear are NOT read from d_x (the active-set convolution need not have written them) but from the
 *         background -- their exact value.  The producer saves the copy of its inactive pixels (61 % of conv2's output),
 *         this kernel the HBM reads of them. */
int svx_bias_relu_pool_lrn(const float* d_x, const float* d_bias, float* d_y, uint32_t n, uint32_t channels,
                           uint32_t height, uint32_t width, int lrn, uint32_t radius, float alpha, float beta,
                           float k, const uint32_t* d_active_rows, const float* d_background, void* stream);

/* Fully connected layer with bias (+ ReLU) on the fp32 matrix cores: out[m][n] = act(bias[n] + sum_k x[m][k] * W[n][k]).
 * Replaces tf.nn.xw_plus_b + relu of fc6 / fc7 (reference src/network/alexnet.py:49-55 via :141-155).
 *   d_x        float32 [m][k] row major
 *   d_w_packed float32 [n/32][k/8][32][8]: packed[b][q][l][j] = W[32 b + l][8 q + j], W = the checkpoint's
 *              [k][n] tensor transposed -- packed once per model (a wave's weight loads are one contiguous stream)
 *   d_out      float32 [m][n]
 *   d_ws       scratch of svx_fc_ws_bytes(m, n, k) bytes (split-K partial sums, added in fixed order: results are
 *              bit-reproducible), 16-byte aligned
 * Requires n % 32 == 0, k % 8 == 0, k >= 192, 16-byte aligned pointers, tensors below 2 GB. */
size_t svx_fc_ws_bytes(uint32_t m, uint32_t n, uint32_t k);
int svx_fc_bias_act(const float* d_x, const float* d_w_packed, const float* d_bias, float* d_out, float* d_ws,
                    uint32_t m, uint32_t n, uint32_t k, int relu, void* stream);

/* fc8 + softmax + argmax in one launch: logits = x @ W^T + b (tf xw_plus_b, src/network/alexnet.py:58,148),
 * tf.nn.softmax and tf.argmax as fetched at src/network/predict.py:209.
 *   d_x [n][4096] fc7 activations, d_w [5][4096] (fc8/weights transposed), d_bias [5]
 *   d_out [n][12] = softmax[5], class (as float), logits[5], 0 */
int svx_fc8_softmax(const float* d_x, const float* d_w, const float* d_bias, float* d_out, uint32_t n, void* stream);

/* fp32 implicit-GEMM convolution on the matrix cores (v_mfma_f32_32x32x2_f32): stride 1, SAME padding,
 * square kernel 3 or 5, optional channel groups, optional fused bias + ReLU.
 * Replaces tf.nn.conv2d (+ split/concat for groups, + bias_add + relu) of the reference layers conv2..conv5
 * (src/network/alexnet.py:34,39,42,45 via :109-135).
 *   d_in       C8 float32 [n][cin/8][height][width][8]
 *   d_w_packed float32 [ksize][ksize][cin_g/8][cout][8], cin_g = cin/groups: the checkpoint tensor
 *              (HWIO [ksize][ksize][cin_g][cout]) with its input-channel axis split into octets and the octet's 8
 *              channels moved innermost -- packed[ky][kx][q][o][j] = hwio[ky][kx][8q + j][o] -- once per model
 *   d_bias     float32 [cout] or NULL (raw convolution output, e.g. in front of svx_bias_relu_pool_lrn)
 *   d_out      C8 float32 [n][cout/8][height][width][8]
 *   d_pixels, d_pixel_count: NULL, or a permutation of all n*H*W output pixel ids (image * H*W + y * W + x) and, in
 *             device memory, the number of leading entries that are active (svx_alexnet_active_sets): only those
 *             outputs are computed (all of them when they are more than 97 %)
 *   d_background: NULL (the other pixels of d_out are left as they are) or C8 float32 [cout/8][height][width][8], the
 *             layer's response to an empty image, copied to the pixels behind the active ones
 * Requires cin_g % 16 == 0, (cout/groups) % 64 == 0, 16-byte aligned pointers, input and weight tensors below 2 GB. */
int svx_conv2d_same(const float* d_in, const float* d_w_packed, const float* d_bias, float* d_out, uint32_t n,
                    uint32_t cin, uint32_t cout, uint32_t height, uint32_t width, uint32_t ksize,
                    uint32_t groups, int relu, const int32_t* d_pixels, const uint32_t* d_pixel_count,
                    const float* d_background, void* stream);

/* One network pass per distinct similarity image of a launch.  An image depends only on the two line set-ups the
 * rasteriser derives from a record (fp64 scaling, clipLine, LineIterator set-up) and the two strand flags; records
 * that agree on them give the same bit planes.
 *   d_records [n][12] int32 as for svx_rasterize
 *   d_unique  out [n][12]: the first occurrence of every distinct image, in input order, in rows [0, *d_live); the
 *             rows behind them repeat record 0 (a consumer without the live count still computes valid images)
 *   d_inv     out [n]: the row of d_unique that holds record i's image
 *   d_live    out, device [1]: the number of distinct images (>= 1 when n >= 1)
 *   d_keys    NULL, or out [n][4] uint32 (16-B aligned): the exact 128-bit image key of every record -- the two Lines
 *             (x0 | y0 << 8 | dx << 16 | dy << 24 each), (sy < 0) | steep << 1 | rev << 2 per line in bytes 0 and 1 of
 *             the third word, count0 | count1 << 16 -- equal keys, equal images; no hash
 *   d_ws      scratch, 4 * n bytes
 * Deterministic (no atomics); n <= 2^26. */
int svx_image_dedup(const int32_t* d_records, uint32_t n, int32_t* d_unique, uint32_t* d_inv, uint32_t* d_live,
                    uint32_t* d_keys, uint32_t* d_ws, void* stream);

/* d_dst[i][c] = d_src[d_inv[i]][c] for i < n, c < width (float32 rows): the packed results of the distinct images
 * expanded to one row per record of the launch. */
int svx_gather_rows(const float* d_src, const uint32_t* d_inv, float* d_dst, uint32_t n, uint32_t width, void* stream);

/* Live-count variants of the CNN stage: as the functions without the suffix, plus d_live (NULL, or a device count of
 * the leading images to compute, e.g. svx_image_dedup's).  Rows >= *d_live are neither read nor written (their
 * outputs keep whatever they held); the launch geometry -- and with it every per-row result, bit for bit, including
 * the split-K grouping of svx_fc_bias_act, which is a function of m -- stays that of n / m.  svx_alexnet_active_sets_live
 * builds the lists over the live images only (d_counts and the pixel totals count those; the image total of d_totals
 * still adds n), and svx_conv2d_same_live (list mode only) follows, and back-fills, those images' pixels only. */
int svx_encode_conv1_live(const int32_t* d_records, uint32_t n, const float* d_w1, const float* d_base, float* d_y,
                          int lrn, uint32_t radius, float alpha, float beta, float k, uint32_t* d_touched,
                          const uint32_t* d_live, void* stream);
int svx_alexnet_active_sets_live(const uint32_t* d_touched, uint32_t n, int32_t* d_list2, int32_t* d_list3,
                                 int32_t* d_list4, int32_t* d_list5, uint32_t* d_counts, uint32_t* d_ws,
                                 uint64_t* d_totals, uint32_t* d_active2, const uint32_t* d_live, void* stream);
int svx_conv2d_same_live(const float* d_in, const float* d_w_packed, const float* d_bias, float* d_out, uint32_t n,
                         uint32_t cin, uint32_t cout, uint32_t height, uint32_t width, uint32_t ksize,
                         uint32_t groups, int relu, const int32_t* d_pixels, const uint32_t* d_pixel_count,
                         const float* d_background, const uint32_t* d_live, void* stream);
int svx_bias_relu_pool_lrn_live(const float* d_x, const float* d_bias, float* d_y, uint32_t n, uint32_t channels,
                                uint32_t height, uint32_t width, int lrn, uint32_t radius, float alpha, float beta,
                                float k, const uint32_t* d_active_rows, const float* d_background,
                                const uint32_t* d_live, void* stream);
int svx_fc_bias_act_live(const float* d_x, const float* d_w_packed, const float* d_bias, float* d_out, float* d_ws,
                         uint32_t m, uint32_t n, uint32_t k, int relu, const uint32_t* d_live, void* stream);
int svx_fc8_softmax_live(const float* d_x, const float* d_w, const float* d_bias, float* d_out, uint32_t n,
                         const uint32_t* d_live, void* stream);

/* (ABI 420, additive) The tail of the memo's chain in one launch.  svx_fc_partial_live is the split-K half of
 * svx_fc_bias_act_live: it leaves the svx_fc_splits(m, n, k) partial sums in d_ws as [split][m][n] and adds nothing up.
 * With m > 64 and a live count its wave tile follows *d_live (32 x 32 up to 64 live rows, the tile of m beyond); the split count and every element's order of summation stay those of m, so the rows are the same bit for bit.
 * svx_fc8_tail_live takes fc7's partial sums [splits][m][4096]: per live row relu(d_bias7 + part[0] + part[1] + ...) in that
 * order (what svx_fc_bias_act_live writes to d_out), svx_fc8_softmax on it, and the packed row written to d_out[i] of every
 * record i < n with d_inv[i] == row (svx_gather_rows; records whose d_inv is not below the live count keep what they held). */
uint32_t svx_fc_splits(uint32_t m, uint32_t n, uint32_t k);
int svx_fc_partial_live(const float* d_x, const float* d_w_packed, float* d_ws, uint32_t m, uint32_t n, uint32_t k,
                        const uint32_t* d_live, void* stream);
int svx_fc8_tail_live(const float* d_part, uint32_t splits, const float* d_bias7, const float* d_w, const float* d_bias,
                      const uint32_t* d_inv, float* d_out, uint32_t m, uint32_t n, const uint32_t* d_live, void* stream);

/* Pairwise signature distances of the clustering step, all partitions of a window in one launch (fp64).
 * Replaces the Python-callback pdist inside linkage(data, method="average", metric=span_position_distance)
 * (reference src/collection/cluster_signatures.py:114 with the metric of :132-141):
 *   d(a, b) = min(|s_a - s_b|, |e_a - e_b|, |floor((s_a+e_a)/2) - floor((s_b+e_b)/2)|) / normalizer
 *             + |span_a - span_b| / max(span_a, span_b)          (NaN when both spans are 0, as NumPy's 0/0)
 *   d_start, d_end  [part_off[n_parts]] signature tstart / tend as doubles, partitions concatenated
 *   d_part_off      [n_parts + 1] first signature of every partition
 *   d_out_off       [n_parts + 1] first output element of every partition; partition p of n signatures owns
 *                   n (n - 1) / 2 doubles in scipy's condensed (pdist) order: (0,1), (0,2), ..., (1,2), ...
 *   total_pairs     = d_out_off[n_parts] (host copy, sizes the grid)
 *   d_out           [total_pairs] */
int svx_span_position_distance(const double* d_start, const double* d_end, const uint64_t* d_part_off,
                               uint32_t n_parts, const uint64_t* d_out_off, uint64_t total_pairs,
                               double normalizer, double* d_out, void* stream);

/* k-mer seed-and-extend of the --hash re-aligner, a batch of independent jobs per launch (integer-exact).
 * Replaces the two HashAligner.run passes of hashplot_unmapped (reference src/segmentplot/run_hash_lineplot.py:70-78:
 * makePairwiseAlignment, extendKmersForward / extendKmersReverse, src/segmentplot/hash_aligner.py:145-239, :37-99) up to
 * the raw hit lists; the self-repeat filter, the collinear merge and select_longest stay on the host.
 * Job = (x: the unmapped read piece, y: its reference window), bases packed one per byte as 4-bit symbols:
 * 0..4 = A C G T N, 5..9 = a c g t n, 10..14 = R Y K M S (upstream's k-mers are raw strings: a symbol matches only
 * itself, only upper-case ACGT complement to something else than N, only 'N' stops an extension); a sequence with
 * any other character must be sent down the host path.  For every job the launch writes, in the reference's loop order
 * (y position ascending, then the k-mer's position list: forward positions ascending, then reverse-strand ones):
 *   list A  hits of y against itself for the k-mers of y that occur once among y's k-mers of both strands
 *   list B  hits of x (both strands) on y for the k-mers of y that are not "avoided" (occur once in y)
 * each hit = int32[4] {y position, x position (forward) or position in the reverse complement, match length, forward}
 * with length >= window; d_counts[2 j], d_counts[2 j + 1] = the numbers of hits of job j (they may exceed hit_cap:
 * the lists are then truncated and the caller must redo the job on the host).
 *   d_table  scratch, 16 bytes per slot, sum of table_slots slots; contents ignored
 * Requires repeat_thresh = 2 and mismatchNum = 0 (what hashplot_unmapped passes), 2 <= k <= 13, x_len <= max_x_len <= 2048;
 * a job with x_len > 2048 is left alone (svx_hash_seeds_long below takes it). */
typedef struct SvxHashJob {
    uint64_t x_off, y_off;       /* byte offsets of the two sequences in d_bases                      */
    uint32_t x_len, y_len;
    uint64_t table_off;          /* first scratch slot of the job                                        */
    uint32_t table_slots;        /* power of two >= 8 * y_len                                            */
    uint32_t hit_cap;            /* capacity of each of the job's two hit lists                         */
    uint64_t hit_off;            /* first hit record of the job: list A at hit_off, list B at + hit_cap */
} SvxHashJob;
int svx_hash_seeds(const uint8_t* d_bases, const SvxHashJob* d_jobs, uint32_t n_jobs, uint64_t* d_table,
                   int32_t* d_hits, uint32_t* d_counts, uint32_t k, uint32_t window, uint32_t max_x_len, void* stream);
/* (ABI 420, additive) The hit lists of a batch, compacted for the read-back: enqueued behind svx_hash_seeds on the same
 * stream, with the same d_jobs / d_hits / d_counts.  The 2 n_jobs lists are numbered A0 B0 A1 B1 ...; a list whose count
 * exceeds its hit_cap holds no row here (d_counts still tells: the caller redoes that job on the host).
 *   d_row_off   [2 n_jobs + 1]  rows in front of every list; the last entry is the total
 *   d_packed    [packed_cap][4] every list's rows, in list order and in their own order; 16-byte aligned, like d_hits
 * Rows behind packed_cap are not written: a caller that reads d_row_off[2 n_jobs] > packed_cap calls again with a larger
 * array (d_hits is untouched, the seeds are not repeated). */
int svx_hash_pack_hits(const SvxHashJob* d_jobs, uint32_t n_jobs, const int32_t* d_hits, const uint32_t* d_counts,
                       uint32_t* d_row_off, int32_t* d_packed, uint64_t packed_cap, void* stream);
/* (ABI 420, additive) svx_hash_seeds for pieces of 2,049 .. 65,536 bases: the same two lists per job, in the same order and
 * record form, into the same d_hits / d_counts through the same SvxHashJob and d_table.  x's k-mer entries are sorted in
 * tiles of 4,096 (the short kernel's LDS table) that are kept in a per-job workspace, so a job needs
 * svx_hash_seeds_long_ws_bytes(x_len, y_len) = 16 x_len + 4 y_len bytes (rounded up to 16) of d_ws, at byte offset
 * d_ws_off[j] (a multiple of 16; d_ws 16-byte aligned; contents ignored).  A batch's short and long jobs share one index space:
 * launch svx_hash_seeds and svx_hash_seeds_long over the same d_jobs range -- this kernel leaves jobs with x_len <= 2048 (and
 * their d_counts, d_ws_off) alone, svx_hash_seeds leaves those with x_len > 2048 alone.
 * Requires 2 <= k <= 13, x_len <= max_x_len <= 65536. */
size_t svx_hash_seeds_long_ws_bytes(uint32_t x_len, uint32_t y_len);
int svx_hash_seeds_long(const uint8_t* d_bases, const SvxHashJob* d_jobs, uint32_t n_jobs, uint64_t* d_table,
                        int32_t* d_hits, uint32_t* d_counts, void* d_ws, const uint64_t* d_ws_off,
                        uint32_t k, uint32_t window, uint32_t max_x_len, void* stream);

/* ---- host side: native BGZF/BAM ingestion (no device work) -------------------------------------------
 * Replaces the per-record pysam iteration of the reference (aln_file.fetch at
 * src/collection/run_collection.py:23-26, field reads at src/collection/collect_signatures.py:128-155):
 * the file is streamed in chunks of BGZF blocks (block-parallel inflate) and the records' fields are appended to
 * packed arrays; SEQ is kept only on request, QUAL and tags never (resident size = the arrays, not the file).
 *   svx_bam_open    -> opaque handle or NULL (svx_bam_error() tells why); threads <= 0: all cores (max 128);
 *                      flags: SVX_BAM_KEEP_SEQ keeps the 4-bit read bases (the --hash re-aligner needs them)
 *   svx_bam_sizes   -> sizes[8] = n_records, n_cigar_words, n_refs, n_names, names_bytes, header_bytes,
 *                      ref_names_bytes, seq_bytes
 *   svx_bam_export  -> fills tid/pos/flag/mapq/l_seq/name_id [n_records], cig_off [n_records+1], cigar
 *                      [n_cigar_words], names / ref_names ('\n'-separated, first-occurrence order), header text,
 *                      ref_lens [n_refs], and (if not NULL) seq_off = byte offset of each record's 4-bit SEQ
 *                      inside the pool exposed by svx_bam_seq() (seq_bytes long) */
#define SVX_BAM_KEEP_SEQ 1
void*          svx_bam_open(const char* path, int threads, int flags);
/* only the records between two BGZF virtual offsets taken from the .bai index (one chromosome = one rank's shard;
 * replaces AlignmentFile.fetch(chrom, ...) random access, run_collection.py:26); voff_end <= voff_beg: header only */
void*          svx_bam_open_range(const char* path, int threads, int flags, uint64_t voff_beg, uint64_t voff_end);
const char*    svx_bam_error(void);
void           svx_bam_sizes(void* handle, uint64_t* sizes);
void           svx_bam_export(void* handle, int threads, int32_t* tid, int32_t* pos, uint16_t* flag, uint8_t* mapq,
                              int32_t* l_seq, int32_t* name_id, int64_t* cig_off, uint32_t* cigar, char* names,
                              char* header, char* ref_names, int32_t* ref_lens, int64_t* seq_off);
const uint8_t* svx_bam_seq(void* handle);
void           svx_bam_close(void* handle);

/* BGZF inflate on the device (svx_inflate2.hip).  Replaces the host-side DEFLATE decoding of htslib / pysam behind
 * run_collection.py:23-26 where host cores are the scarce resource.  d_comp: the compressed bytes as they sit in the file
 * (16-byte aligned -- SVX_EINVAL otherwise --, readable up to the next multiple of 16 behind the last payload); d_src_off /
 * d_src_len [n]: byte offset in d_comp and size of every block's DEFLATE payload (behind the block header, in front of CRC32 +
 * ISIZE); d_dst_off [n + 1]: running sum of the ISIZE fields = where every block's bytes go in d_out; d_status [n]: 0 = the
 * block inflated to exactly ISIZE bytes, anything else = corrupt (the caller falls back to the host decoder).
 * Two kernels: (A) one WAVE per block decodes the Huffman code in parallel -- 64
 * segments of the compressed bits per step, every lane from its segment's first bit, re-synchronised with its predecessor --
 * and transcodes the tokens into a byte-aligned LZ sequence stream; (B) one LANE per block copies literals and matches
 * from that stream.  inflated_bytes: d_dst_off[n] - d_dst_off[0] (the caller summed the ISIZE fields on the host).  d_ws: at least
 * svx_bgzf_inflate_fast_ws_bytes(inflated_bytes, n) bytes (16-byte aligned; SVX_EINVAL if ws_bytes is less) for the
 * sequence streams.  Same statuses; blocks whose stream would not fit its slot (pathological: hundreds of tiny DEFLATE
 * blocks) are decoded by the wave-per-block kernel inside the call. */
size_t         svx_bgzf_inflate_fast_ws_bytes(uint64_t inflated_bytes, uint32_t n_blocks);
int            svx_bgzf_inflate_fast(const uint8_t* d_comp, const uint64_t* d_src_off, const uint32_t* d_src_len,
                                     const uint64_t* d_dst_off, uint32_t n_blocks, uint64_t inflated_bytes, uint8_t* d_out,
                                     uint32_t* d_status, void* d_ws, uint64_t ws_bytes, void* stream);
/* The same with kernel A on stream_tokens and kernel B (and whatever follows in the caller's order: the CRC, the record walk)
 * on stream_lz, which waits for A through an event.  A caller with several launches in flight puts every A on ONE stream:
 * the tokens kernels own the chip while they run, so two of them launched side by side on two streams finish together --
 * late --, while one after the other the first launch's blocks go on to their LZ copies (latency-bound, next to the second
 * launch's A) a whole A earlier.  stream_tokens == stream_lz: svx_bgzf_inflate_fast. */
int            svx_bgzf_inflate_fast_on(const uint8_t* d_comp, const uint64_t* d_src_off, const uint32_t* d_src_len,
                                        const uint64_t* d_dst_off, uint32_t n_blocks, uint64_t inflated_bytes, uint8_t* d_out,
                                        uint32_t* d_status, void* d_ws, uint64_t ws_bytes, void* stream_tokens, void* stream_lz);
/* CRC32 of every inflated block against the block's footer -- the four bytes behind its DEFLATE payload in d_comp (RFC 1952
 * 2.3.1) -- what htslib checks on every block behind pysam's fetch (/root/reference/src/collection/run_collection.py:23-26).
 * d_out / d_dst_off / d_comp / d_src_off / d_src_len: as svx_bgzf_inflate_fast took and wrote them.  d_status [n]: left alone where
 * the CRC agrees or a status is already set, SVX_INFLATE_BAD_CRC where it differs.  One wave per block, coalesced dword
 * reads, one LDS look-up per byte (svx_crc.hip). */
#define SVX_INFLATE_BAD_CRC 9
int            svx_bgzf_crc32(const uint8_t* d_out, const uint64_t* d_dst_off, const uint8_t* d_comp, const uint64_t* d_src_off,
                              const uint32_t* d_src_len, uint32_t n_blocks, uint32_t* d_status, void* stream);
/* BAM records in an inflated stream on the device -> packed arrays (svx_bamdev.hip).  d_starts [n_starts + 1]: byte
 * offsets in d_raw of known record starts (from the .bai linear index), ascending, the last entry = end of the part.
 *   svx_bam_walk_count    d_counts [n_starts][4] = records, CIGAR words, QNAME bytes (one separator per record) between
 *                         start i and start i + 1, and a status: 0 ok, 1 the walk misses the next start, 2 malformed
 *                         record.  A CIGAR of more than 65,535 operations is read from the record's CG:B,I tag
 *                         (SAMv1 4.2.2), by both passes
 *   svx_bam_walk_extract  d_base [n_starts][3] = exclusive prefix sums of the first three counts; fills tid / pos / flag /
 *                         mapq / l_seq [records], cig_off / name_off [records + 1] (offsets of each record's words / name;
 *                         the closing entry = the totals: ABI 370, the caller appended it before),
 *                         cigar [words], names [bytes] ('\n' behind every name).  n_records = the sum of the records counts
 *                         (ABI 420: a lane per start notes where every record lies, a wave per record copies it -- d_tid / d_pos
 *                         carry the record's byte offset between the two launches; d_raw is read in aligned dwords: readable
 *                         up to the next multiple of 4 behind its last byte) */
int            svx_bam_walk_count(const uint8_t* d_raw, const uint64_t* d_starts, uint32_t n_starts, uint64_t* d_counts, void* stream);
int            svx_bam_walk_extract(const uint8_t* d_raw, const uint64_t* d_starts, uint32_t n_starts, const uint64_t* d_base,
                                    int32_t* d_tid, int32_t* d_pos, uint16_t* d_flag, uint8_t* d_mapq, int32_t* d_l_seq,
                                    int64_t* d_cig_off, uint32_t* d_cigar, int64_t* d_name_off, uint8_t* d_names, uint32_t n_records,
                                    void* stream);
/* The same walk WITH the read bases (--hash / --graph on the device engine); the two exports above are untouched by it.
 *   svx_bam_walk_count_seq    as svx_bam_walk_count, and d_seq_bytes [n_starts] = the SEQ bytes -- (l_seq + 1) / 2 a record --
 *                             between start i and start i + 1
 *   svx_bam_walk_extract_seq  as svx_bam_walk_extract, and d_seq_base [n_starts] = exclusive prefix sum of d_seq_bytes;
 *                             fills d_seq_off [records + 1] (dense, as the host decoder builds it; the closing entry = the
 *                             total) and d_seq [total]: every record's 4-bit SEQ as stored in the file, the spare nibble of
 *                             an odd length included.  A wave per record, 16-byte stores aligned on d_seq, whole chunks only
 *                             where they hold no neighbour's byte.  d_raw must be 16-byte aligned and readable up to the
 *                             next multiple of 16 behind its last byte (aligned 16-byte loads) */
int            svx_bam_walk_count_seq(const uint8_t* d_raw, const uint64_t* d_starts, uint32_t n_starts, uint64_t* d_counts,
                                      uint64_t* d_seq_bytes, void* stream);
int            svx_bam_walk_extract_seq(const uint8_t* d_raw, const uint64_t* d_starts, uint32_t n_starts, const uint64_t* d_base,
                                        int32_t* d_tid, int32_t* d_pos, uint16_t* d_flag, uint8_t* d_mapq, int32_t* d_l_seq,
                                        int64_t* d_cig_off, uint32_t* d_cigar, int64_t* d_name_off, uint8_t* d_names,
                                        const uint64_t* d_seq_base, int64_t* d_seq_off, uint8_t* d_seq, uint32_t n_records,
                                        void* stream);
/* Record starts WITHOUT an index (svx_bamindex.hip): a BAM that has no .bai names one record start -- the end of its header --
 * and chains the others through their block_size fields.  For a range of whole BGZF blocks inflated to d_raw (d_dst_off [n_blocks + 1]:
 * where every block's bytes lie, as svx_bgzf_inflate_fast took them) and `entry`, the byte offset in d_raw of one known record start
 * (d_dst_off[0] <= entry <= d_dst_off[n_blocks]: the header's end in a file's first range, d_exit[0] of the range in front in a later one):
 *   d_first [n_blocks]  the offset in d_raw of the first record of the chain from `entry` that STARTS in block b, UINT64_MAX
 *                       where none does (a block inside one long record, a block in front of `entry`, a block of no bytes)
 *   d_exit [2]          [0] the start of the chain's last record where the range's end cuts it, the range's end where the
 *                       chain ends exactly there; [1] status: 0 ok, 1 the chain ran into a malformed record, at offset [0]
 *   n_ref, d_ref_len    the reference dictionary (int32 lengths): what a plausible record may name
 *   d_ws                scratch of ws_bytes >= svx_bam_find_starts_ws_bytes(n_blocks) bytes, 16-byte aligned, contents ignored
 * A wave per block guesses the block's first start (64 offsets a step, the lowest that looks like a record) and walks from it
 * to the block's end; a guess counts only if the chain from `entry` arrives exactly on it -- pointer doubling over the blocks'
 * successor links marks that path in log2(n_blocks) launches, and one lane re-walks the block behind every link that does not
 * hold: serial work per broken link, not per block or record.  No atomics; the result does not depend on the guesses.
 * The compacted d_first + d_exit[0] is the d_starts array of svx_bam_walk_count / svx_bam_walk_extract (2 + 2 log2(n_blocks) launches).
 *   svx_bam_walk_offsets  d_rec_off [records] = the byte offset in d_raw of every record between the starts, in the order and
 *                       with the d_base of svx_bam_walk_extract (a lane per start; after a count pass with status 0) */
size_t         svx_bam_find_starts_ws_bytes(uint32_t n_blocks);
int            svx_bam_find_starts(const uint8_t* d_raw, const uint64_t* d_dst_off, uint32_t n_blocks, uint64_t entry, uint32_t n_ref,
                                   const int32_t* d_ref_len, uint64_t* d_first, uint64_t* d_exit, void* d_ws, uint64_t ws_bytes,
                                   void* stream);
int            svx_bam_walk_offsets(const uint8_t* d_raw, const uint64_t* d_starts, uint32_t n_starts, const uint64_t* d_base,
                                    uint64_t* d_rec_off, void* stream);
/* The records of an UNSORTED BAM in coordinate order (svx_recsort.hip; ABI 420, additive): the walk above takes a file apart in
 * file order, these put its arrays into the order of `samtools sort`.
 *   svx_record_sort     d_order [n]: d_order[r] = the input index of the record of sorted rank r, by the key
 *                       ((tid < 0 ? n_ref : tid) << 32) | (uint32)(pos + 1) ascending -- records without a reference last --,
 *                       STABLE: records of equal key keep their input order.  d_tid / d_pos [n] int32, pos >= -1.  pos_bits
 *                       (1 .. 32): the significant bits of pos + 1, bit_length(longest reference + 1); higher bits of pos + 1
 *                       are ignored.  An LSD radix sort, 8 bits a pass, over pos_bits + bit_length(n_ref) bits: per pass a
 *                       histogram per tile of SVX_RECORD_SORT_TILE records, one scan of the 256 x tiles table, a scatter
 *                       whose in-tile ranks come from wave ballots and LDS counters, lanes and waves taken in order.
 *                       d_ws: ws_bytes >= svx_record_sort_ws_bytes(n) (20 bytes a record + the table), 16-byte aligned
 *   svx_record_gather   d_dst[r] = d_src[d_order[r]] for n elements of elem_bytes 1, 2 or 4 (tid, pos, flag, mapq, l_seq);
 *                       both arrays aligned to elem_bytes
 *   svx_record_gather_offsets   d_off_out [n + 1] = the exclusive prefix sum (int64) of the lengths d_off_in[s + 1] - d_off_in[s]
 *                       taken in the order s = d_order[0], d_order[1], ...; the closing entry = the total.  d_off_in [n + 1].
 *                       d_ws: ws_bytes >= svx_record_gather_offsets_ws_bytes(n), 16-byte aligned
 *   svx_record_gather_segments  segment d_order[r] of d_src -- elements d_off_in[s] .. d_off_in[s + 1] of elem_bytes 1, 2 or 4 --
 *                       copied to element d_off_out[r] of d_dst, a wave per record; segments of no element and of more than
 *                       65,535 are fine.  4 for CIGAR words, 1 for QNAME bytes (the '\n' behind a name belongs to its
 *                       segment) and for SEQ bytes (byte-aligned per record, as svx_bam_walk_extract_seq writes them).
 *                       d_src is read in aligned dwords: 4-byte aligned, readable up to the next multiple of 4 behind its last
 *                       byte; d_dst aligned to elem_bytes.  Exactly the total's bytes of d_dst are written: the 4 readable
 *                       words svx_cigar_scan wants behind a gathered CIGAR array are the caller's to allocate.
 *   svx_record_invert   d_rank [n]: d_rank[d_order[r]] = r, the sorted rank of every input record (a thread per element)
 *   svx_record_scatter_segments  the gather turned round, for an output stream that is filled in pieces (svision_amd/sort.py: a
 *                       file whose records do not fit the device).  n INPUT records lie in d_src at the byte offsets
 *                       d_src_off [n + 1]; d_rank [n] are their ranks in the whole output, d_off_out that output's offsets
 *                       (svx_record_gather_offsets: indexed by RANK, entries up to rank_hi are read).  A wave per input record:
 *                       where rank_lo <= d_rank[i] < rank_hi the bytes d_src[d_src_off[i] .. d_src_off[i + 1]) go to
 *                       d_dst + d_off_out[rank] - out_base; the waves of all other records return at once.  The alignment
 *                       rule is the gather's, the destination decides.  d_src is read only in the aligned dwords that hold a
 *                       segment's bytes: 4-byte aligned, readable up to the next multiple of 4 behind its last byte (the
 *                       d_raw of the walk has 16).  d_dst: any alignment; only the bytes of the window's records are written.
 *                       A record whose length d_src_off[i + 1] - d_src_off[i] is not d_off_out[rank + 1] - d_off_out[rank]
 *                       is NOT copied and d_status[0] is set to 1 (a plain store of the one value from any number of waves;
 *                       the caller zeroes it); the other records are copied.  Segments of no byte and of more than 65,535
 *                       bytes are fine; n = 0 and an empty window launch nothing
 *   svx_record_retid    the reference indices of n BAM records rewritten in place through a table (svision_amd/sort.py: several
 *                       inputs merged into one file, d_map [n_in] = every reference index of one input in the merged dictionary).
 *                       Record r starts at d_bytes + d_off[r], at its block_size field -- any byte offset, at least 36 bytes --;
 *                       refID is the little-endian int32 at byte 4, next_refID the one at byte 24.  Each field: -1 stays -1,
 *                       0 <= v < n_in becomes d_map[v]; a record with a field outside that keeps BOTH fields as they are and
 *                       d_status[0] is set to 1 (a plain store of the one value; the caller zeroes it).  d_tid_key [n] (may be
 *                       NULL): the records' sort keys, translated by the same rule.  A lane per record in a grid-stride loop,
 *                       byte loads and stores: only bytes 4..7 and 24..27 of a record are touched, nothing is read behind
 *                       d_off[n - 1] + 28.  n = 0 launches nothing; n_in = 0: every field other than -1 is reported
 *   svx_record_retag_measure / svx_record_retag_write   the value of a record's RG:Z and PG:Z field replaced through a table
 *                       (svision_amd/sort.py under retag: the @RG / @PG IDs of several inputs that collide were renamed in the
 *                       merged header, and the records follow).  Record r = the bytes d_bytes[d_off[r] .. d_off[r + 1]), d_off
 *                       [n + 1], at any byte offset.  The table: m entries, entry e = a 2-byte tag, the old value and the new
 *                       one packed in d_table with the int32 offsets d_table_off [2m + 1]: the tag at d_table_off[2e], the old
 *                       value behind it up to d_table_off[2e + 1], the new one from there up to d_table_off[2e + 2]; values
 *                       carry no NUL; only entries of the tags RG and PG are looked for.  A wave per record walks the optional
 *                       fields behind qual (l_read_name, n_cigar_op and l_seq of the fixed part say where): A c C 1 byte, s S 2,
 *                       i I f 4, Z H up to their NUL (found 64 bytes a ballot), B = subtype + uint32 count + count elements,
 *                       skipped in one step.  The FIRST RG field of type Z whose value equals an RG entry's old value -- same
 *                       length, same bytes -- takes that entry's new value, and likewise PG; a field of the tag with another
 *                       type or a value the table does not hold is left alone, and so is everything else, byte for byte and in
 *                       order.  block_size becomes the new length - 4.  measure: d_new_len[r] (int64) = the new length.  write:
 *                       exactly that many bytes at d_dst + d_new_off[r], d_new_off [n + 1] the exclusive sum of d_new_len, in
 *                       up to five copies (prefix, value, middle, value, rest) by the scatter's copy routine; nothing else of
 *                       d_dst is written.  A MALFORMED record -- shorter than 36 bytes, block_size + 4 not its extent, name +
 *                       CIGAR + seq + qual longer than it, a field header cut by its end, an unknown type or B subtype, a value
 *                       or a B array past the end, a Z / H without NUL -- keeps its length, is copied as it is, and d_status[0] is
 *                       set to 1 (a plain store of the one value; the caller zeroes it); write also sets it, and copies
 *                       nothing of that record, where d_new_off does not give a record the length measure computes.  measure
 *                       reads the records byte by byte and nothing outside d_bytes[d_off[0] .. d_off[n]); write reads d_bytes
 *                       and d_table in aligned dwords as svx_record_scatter_segments reads d_src: both 4-byte aligned and
 *                       readable up to the next multiple of 4 behind their last byte.  n = 0 or m = 0 launches nothing
 *   svx_record_tags_measure / svx_record_tags_write   optional fields removed from every record by their two-byte tag
 *                       (svision_amd/sort.py under drop_tags / keep_tags; ABI 420, additive).  Records, offsets and the walk of
 *                       the fields are those of svx_record_retag_measure, a wave per record.  d_table: a bitmap of
 *                       SVX_RECORD_TAGS_TABLE_BYTES bytes, 4-byte aligned, read as dwords: bit (t0 | t1 << 8) -- bit k of the
 *                       little-endian bitmap is bit k % 32 of dword k / 32 -- set = every field whose tag is the bytes t0 t1 is
 *                       REMOVED, whatever its type and however often it occurs; a keep list is the complement.  The kept
 *                       fields stay in the record's order, everything else of it byte for byte; block_size becomes the new
 *                       length - 4.  measure: d_new_len[r] (int64) = the record's length without the removed fields.  write:
 *                       exactly that many bytes at d_dst + d_new_off[r], d_new_off [n + 1] the exclusive sum of d_new_len: the
 *                       fixed part with the fields in front of the first removed one, and every further maximal run of kept
 *                       fields, is one copy by the scatter's copy routine; nothing else of d_dst is written.  d_status[0]
 *                       (the caller zeroes it; a plain store of the one value): 0 = every record was well formed and, in
 *                       write, every record had the length of its walk; 1 = a MALFORMED record (the list above: it keeps its
 *                       length and is copied as it is), or, in write, d_new_off gives a record another length than its walk
 *                       (nothing of that record is written; the others are).  SLACK: measure reads the records byte by byte
 *                       and nothing outside d_bytes[d_off[0] .. d_off[n]) -- none; write reads d_bytes in aligned dwords as
 *                       svx_record_scatter_segments reads d_src: 4-byte aligned and readable up to the next multiple of 4
 *                       behind its last byte -- at most 3 bytes.  n = 0 launches nothing
 * No atomics in any of them: the output is a pure function of the input.  n = 0 is fine everywhere (d_off_out[0] = 0). */
#define SVX_RECORD_SORT_TILE 2048u
size_t         svx_record_sort_ws_bytes(uint32_t n);
int            svx_record_sort(const int32_t* d_tid, const int32_t* d_pos, uint32_t n, uint32_t n_ref, uint32_t pos_bits,
                               uint32_t* d_order, void* d_ws, uint64_t ws_bytes, void* stream);
int            svx_record_gather(const void* d_src, const uint32_t* d_order, void* d_dst, uint32_t n, uint32_t elem_bytes, void* stream);
size_t         svx_record_gather_offsets_ws_bytes(uint32_t n);
int            svx_record_gather_offsets(const int64_t* d_off_in, const uint32_t* d_order, uint32_t n, int64_t* d_off_out, void* d_ws,
                                         uint64_t ws_bytes, void* stream);
int            svx_record_gather_segments(const void* d_src, const int64_t* d_off_in, const uint32_t* d_order, const int64_t* d_off_out,
                                          void* d_dst, uint32_t n, uint32_t elem_bytes, void* stream);
int            svx_record_invert(const uint32_t* d_order, uint32_t n, uint32_t* d_rank, void* stream);
int            svx_record_scatter_segments(const void* d_src, const int64_t* d_src_off, const uint32_t* d_rank, uint32_t rank_lo,
                                           uint32_t rank_hi, const int64_t* d_off_out, int64_t out_base, void* d_dst, uint32_t n,
                                           int32_t* d_status, void* stream);
int            svx_record_retid(void* d_bytes, const int64_t* d_off, uint32_t n, const int32_t* d_map, int32_t n_in, int32_t* d_tid_key,
                                int32_t* d_status, void* stream);
int            svx_record_retag_measure(const void* d_bytes, const int64_t* d_off, uint32_t n, const void* d_table, const int32_t* d_table_off,
                                        int32_t m, int64_t* d_new_len, int32_t* d_status, void* stream);
int            svx_record_retag_write(const void* d_bytes, const int64_t* d_off, uint32_t n, const void* d_table, const int32_t* d_table_off,
                                      int32_t m, const int64_t* d_new_off, void* d_dst, int32_t* d_status, void* stream);
#define SVX_RECORD_TAGS_TABLE_BYTES 8192u
int            svx_record_tags_measure(const void* d_bytes, const int64_t* d_off, uint32_t n, const uint32_t* d_table, int64_t* d_new_len,
                                       int32_t* d_status, void* stream);
int            svx_record_tags_write(const void* d_bytes, const int64_t* d_off, uint32_t n, const uint32_t* d_table, const int64_t* d_new_off,
                                     void* d_dst, int32_t* d_status, void* stream);
/* BGZF members FROM inflated bytes (svx_deflate.hip; ABI 420, additive): the encoder of svision_amd/sort.py, which writes the
 * device-sorted BAM.
 *   svx_bgzf_deflate    block b = the bytes d_in[d_in_off[b] .. d_in_off[b + 1]) -- any offsets, no alignment, 0 .. 0xFF00 bytes a block --
 *                       becomes ONE complete BGZF member in slot b of d_slots [n_blocks][SVX_BGZF_SLOT]: the 18-byte header (1f 8b 08 04,
 *                       MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 2, BSIZE - 1), one final DEFLATE block, CRC32 of the input (the device
 *                       function svx_bgzf_crc32 checks with), ISIZE.  d_member_len [b] = the member's bytes (a block of more than
 *                       0xFF00 bytes: 0, nothing written), d_stored [b] = 1 where the DEFLATE block is stored.  The block: a greedy
 *                       LZ77 parse -- lengths 3 .. 258, distances 1 .. 32,768, one hash-table candidate and the nearest one in the same
 *                       wave per position -- in the FIXED Huffman code (BTYPE 01), or the bytes stored (BTYPE 00) whenever the fixed
 *                       form would not be smaller: no member is longer than its block + 31 bytes, 65,311 for a full one.  An empty
 *                       block gives the 28-byte BGZF end-of-file marker.  One workgroup per block, block and table in LDS.
 *                       The member's bytes are a pure function of the block's bytes: the same on every run and under every
 *                       scheduling (the LDS atomics are max and or; every other access is ordered by a barrier, but for the parse's
 *                       marks, whose final set is the same in every order: svx_deflate_core.hpp).  The kernel needs 153 KB of
 *                       dynamic LDS; the opt-in is made on the device that is current at the call, once per device
 *   svx_bgzf_pack       d_file_off [n_blocks + 1] = the exclusive prefix sum of d_member_len, computed on the device, the closing entry
 *                       = the file bytes; member b copied from its slot to d_out + d_file_off[b].  A member that would end behind
 *                       out_bytes is not copied: out_bytes >= the inflated bytes + 31 n_blocks always holds them all
 *   svx_bgzf_deflate_dyn  (additive) svx_bgzf_deflate with a third form of the DEFLATE block: the SAME parse, its tokens kept in d_ws
 *                       and counted in LDS, then Huffman codes built in the workgroup from those counts -- literal/length and
 *                       distance codes of at most 15 bits, their lengths run-length coded with 16 / 17 / 18 the way zlib does it, that
 *                       sequence's code of at most 7 bits, HLIT / HDIST / HCLEN trimmed; every code complete (Kraft sum 1, at least two
 *                       symbols: an unused distance alphabet gets two codes of 1 bit) --, the sizes of the three forms counted before a
 *                       bit is written, and the smallest written: the bytes stored at a tie, then the fixed code, then DYNAMIC codes
 *                       (BTYPE 10).  d_btype [b] = 0, 1 or 2, the block's BTYPE.  Where it is 0 or 1 the member is svx_bgzf_deflate's,
 *                       byte for byte; no member is longer than that one.  A block of more than 0xFF00 bytes: length 0, nothing
 *                       written.  Ties between symbols of one count are broken by symbol index and the limit's repair is a fixed rule,
 *                       the LDS atomics are max, or and integer add: the member's bytes are a pure function of the block's bytes.
 *                       d_ws: svx_bgzf_deflate_dyn_ws_bytes(n_blocks) bytes, 8-byte aligned (SVX_EINVAL otherwise) -- 73,440 a block:
 *                       one byte a position, where a match keeps its 23 bits, and one bit a position for the tokens' starts --;
 *                       ws_bytes below that: SVX_ECAPACITY, nothing launched, nothing written.  A workspace with 32 bytes a block to
 *                       spare also receives, behind those bytes, four uint64 a block: the 100 MHz clock at the kernel's start, after
 *                       the parse, after the code construction and at its end (tools/sort_write_time.py).  153 KB of dynamic LDS +
 *                       1,280 bytes for the two histograms; the opt-in as above */
#define SVX_BGZF_SLOT 65536u
#define SVX_BGZF_BLOCK_MAX 0xFF00u
int            svx_bgzf_deflate(const uint8_t* d_in, const uint64_t* d_in_off, uint32_t n_blocks, uint8_t* d_slots, uint32_t* d_member_len,
                                uint32_t* d_stored, void* stream);
size_t         svx_bgzf_deflate_dyn_ws_bytes(uint32_t n_blocks);
int            svx_bgzf_deflate_dyn(const uint8_t* d_in, const uint64_t* d_in_off, uint32_t n_blocks, uint8_t* d_slots, uint32_t* d_member_len,
                                    uint32_t* d_btype, void* d_ws, uint64_t ws_bytes, void* stream);
int            svx_bgzf_pack(const uint8_t* d_slots, const uint32_t* d_member_len, uint32_t n_blocks, uint64_t* d_file_off, uint8_t* d_out,
                             uint64_t out_bytes, void* stream);
/* SAM text -> BAM records (svx_sam.hip over svx_sam_core.hpp; ABI 420, additive): the front end of svision_amd/sort.py for an
 * aligner's text output.  The rules are listed in svision_amd/io/sam.py, which encodes the same bytes on the host.  d_text: a chunk of
 * n_bytes of alignment lines that ends at a line boundary (the last line may lack its newline), with SVX_SAM_SLACK readable bytes
 * behind it.
 *   svx_sam_lines    d_line_off [n_lines + 1]: the offset of every line start and n_bytes behind them (line i = the bytes
 *                    [d_line_off[i], d_line_off[i + 1]) without its newline), *d_n_lines = their number.  A count launch, a prefix of
 *                    the tiles' counts in one workgroup, an emit launch; no atomics.  cap = the entries of d_line_off (>= 1): entries
 *                    beyond it are dropped, *d_n_lines + 1 > cap tells.  d_ws: svx_sam_lines_ws_bytes(n_bytes) bytes, 8-byte aligned
 *   svx_sam_measure  a wave a line: d_len [i] = the bytes of the line's BAM record including block_size, or a negative code;
 *                    d_tid d_pos d_flag d_span [i] = the sort key and the index's fields (where d_len is an error code: unspecified).
 *                    SVX_SAM_HOST: the line is valid as far as the kernel looked and is not taken by it -- more than 65,535 CIGAR
 *                    operations, or an f / B:f value outside the exact fast path (at most 15 significant digits and a decimal
 *                    exponent of magnitude <= 22: one IEEE double multiply or divide, then the cast), inf and nan among them.
 *                    SVX_SAM_E_*: FIELDS fewer than 11 fields or an empty line, NUMBER a numeric field or array value that is no
 *                    number or out of its range, NAME a read name of 0 or more than 254 bytes, RNAME a reference the table does not
 *                    hold, CIGAR, QUAL another length than SEQ, TAG a malformed tag, RANGE an i tag outside [-2^31, 2^32), HEADER a
 *                    line that starts with '@'.  The reference table: d_ref_hash [n_ref] the names' FNV-1a hashes ascending,
 *                    d_ref_tid [n_ref] their tids in that order, d_ref_name_off [n_ref + 1] / d_ref_names the names' bytes by tid;
 *                    the kernel compares the bytes
 *   svx_sam_encode   a wave a line: the record of every line with d_len [i] >= 0 written to d_out + (d_off[i] - out_base), exactly
 *                    d_len [i] bytes -- the resident stream (out_base 0) or a chunk-local buffer.  A line that no longer measures
 *                    d_len [i] is not written: *d_status = 1 (a plain store; zero it before the call).  Lines with d_len [i] < 0 are
 *                    skipped
 * Every loop is bounded by the line table, reads stay inside the chunk and its slack, no kernel waits for another. */
#define SVX_SAM_SLACK 64u
#define SVX_SAM_HOST (-1)
#define SVX_SAM_E_FIELDS (-2)
#define SVX_SAM_E_NUMBER (-3)
#define SVX_SAM_E_NAME (-4)
#define SVX_SAM_E_RNAME (-5)
#define SVX_SAM_E_CIGAR (-6)
#define SVX_SAM_E_QUAL (-7)
#define SVX_SAM_E_TAG (-8)
#define SVX_SAM_E_RANGE (-9)
#define SVX_SAM_E_HEADER (-10)
size_t         svx_sam_lines_ws_bytes(uint64_t n_bytes);
int            svx_sam_lines(const uint8_t* d_text, uint64_t n_bytes, int64_t* d_line_off, uint64_t cap, uint64_t* d_n_lines, void* d_ws,
                             uint64_t ws_bytes, void* stream);
int            svx_sam_measure(const uint8_t* d_text, const int64_t* d_line_off, uint32_t n_lines, const uint32_t* d_ref_hash,
                               const int32_t* d_ref_tid, const uint32_t* d_ref_name_off, const uint8_t* d_ref_names, uint32_t n_ref,
                               int32_t* d_len, int32_t* d_tid, int32_t* d_pos, int32_t* d_flag, int32_t* d_span, void* stream);
int            svx_sam_encode(const uint8_t* d_text, const int64_t* d_line_off, uint32_t n_lines, const uint32_t* d_ref_hash,
                              const int32_t* d_ref_tid, const uint32_t* d_ref_name_off, const uint8_t* d_ref_names, uint32_t n_ref,
                              const int32_t* d_len, const int64_t* d_off, int64_t out_base, uint8_t* d_out, int32_t* d_status, void* stream);
/* SAM text -> the caller's packed arrays (svx_sam.hip over svx_sam_core.hpp; ABI 420, additive): the front end of
 * svision_amd/ingest_sort.py for text, a pipe and several inputs.  No BAM record is built: a chunk's lines become what
 * svx_bam_walk_extract(_seq) writes for the same records.  d_text, d_line_off and the reference table as above; a wave a line, a
 * bounded grid whose waves stride over the lines.
 *   svx_sam_pack_count    d_status [i] = 0, SVX_SAM_HOST, or the SVX_SAM_E_* code svx_sam_measure gives for the same fault in the
 *                         first eleven fields.  The tags are not read (a malformed tag refuses no line here), QUAL is held to SEQ's
 *                         length and not read, and the number of CIGAR operations has no limit.  SVX_SAM_HOST, the only one of these
 *                         kernels: a CIGAR of the shape <l_seq>S<n>N, the placeholder beside a CG:B:I tag -- the caller encodes that
 *                         line on the host and puts its counts and bytes into the line's own slots.  d_fields: five planes of
 *                         n_lines (tid, pos, flag, mapq, l_seq), d_counts: three (CIGAR words, name bytes = the name + one '\n',
 *                         SEQ bytes = (l_seq + 1) / 2, 0 without with_seq); zero where d_status [i] is not 0
 *   svx_sam_pack_extract  d_cig_off d_name_off d_seq_off [n_lines + 1]: the exclusive prefix of the counts (the caller's; a line it
 *                         took on the host has its counts in it).  Every line with d_status [i] == 0: d_tid d_pos d_l_seq d_flag
 *                         d_mapq [i], its words to d_cigar + d_cig_off [i], its name and the '\n' to d_names + d_name_off [i], its
 *                         4-bit SEQ as BAM stores it (the spare nibble of an odd length zero) to d_seq + d_seq_off [i] -- byte-aligned
 *                         neighbours, single byte stores.  d_seq and d_seq_off both NULL: no bases.  Every store is checked against the
 *                         record's own slot [off [i], off [i + 1]); other lines are skipped and their elements left as they are
 * No atomics, every loop bounded by the line's bytes, reads inside the chunk and its slack. */
int            svx_sam_pack_count(const uint8_t* d_text, const int64_t* d_line_off, uint32_t n_lines, const uint32_t* d_ref_hash,
                                  const int32_t* d_ref_tid, const uint32_t* d_ref_name_off, const uint8_t* d_ref_names, uint32_t n_ref,
                                  int with_seq, int32_t* d_status, int32_t* d_fields, int32_t* d_counts, void* stream);
int            svx_sam_pack_extract(const uint8_t* d_text, const int64_t* d_line_off, uint32_t n_lines, const uint32_t* d_ref_hash,
                                    const int32_t* d_ref_tid, const uint32_t* d_ref_name_off, const uint8_t* d_ref_names, uint32_t n_ref,
                                    const int32_t* d_status, int32_t* d_tid, int32_t* d_pos, int16_t* d_flag, uint8_t* d_mapq, int32_t* d_l_seq,
                                    const int64_t* d_cig_off, uint32_t* d_cigar, const int64_t* d_name_off, uint8_t* d_names,
                                    const int64_t* d_seq_off, uint8_t* d_seq, void* stream);
/* host helpers of the device-side ingestion: parallel positional read into caller memory; the whole BGZF blocks of a
 * buffer (payload offset / size, ISIZE, file offset; -> their number or -1, *used = bytes they cover); QNAME ids by
 * first occurrence (-> number of distinct names, written '\n'-separated to uniq) */
int            svx_read_range(const char* path, uint64_t off, uint64_t n, uint8_t* dst, int threads);
int64_t        svx_bgzf_index(const uint8_t* bytes, uint64_t n, uint64_t base_coff, uint64_t cap, uint64_t* src_off,
                              uint32_t* src_len, uint32_t* isize, uint64_t* coff, uint64_t* used);
int64_t        svx_name_ids(const uint8_t* names, const int64_t* name_off, uint64_t n, int32_t* name_id, uint8_t* uniq,
                            uint64_t* uniq_bytes);

/* The staging reader of the device-side ingestion (svx_stage.hip over svx_stage_core.hpp; ABI 420, additive): the file ranges
 * of a run's groups go through a ring of the caller's pinned slots to the device.  One descriptor and one pool of pread threads
 * per handle, alive from open to close; a slot is 65,536 bytes of head-room + payload, filled at fixed file offsets (the head of
 * a block cut by a slot's end is carried to the head-room of the next one), so the reads run ahead of the index and into the
 * next range as far as slots are free.  Every HIP call is made by the calling thread.
 *   svx_stage_open    ranges = n_ranges pairs [c0, c1) of file offsets, each c0 at a BGZF block; slot_ptrs = n_slots (>= 2) host
 *                     addresses of slot_bytes (>= 131,072) each, not touched by anyone else until the close; copy_stream = the
 *                     hipStream_t the uploads go to.  -> opaque handle or NULL (svx_bam_error tells why)
 *   svx_stage_group   the next range, completely: per slot wait for its bytes, carry, index, hipMemcpyAsync of the whole blocks
 *                     to d_comp + (the block's file offset - c0) and the slot's event behind it.  -> the number of whole blocks
 *                     of the range (>= 1), *used = the bytes they cover, waits [3] = seconds the call waited for bytes / for a
 *                     slot's earlier copy / took in all, stamps [2 x up to stamps_cap] = per slot the seconds since the open at
 *                     which its bytes were there and its copy was enqueued (may be NULL) -- or, with the text in svx_bam_error,
 *                     -1 bad argument, -2 read error or a range past the end of the file, -3 no BGZF block at the start of the
 *                     range, -4 not BGZF further inside, -5 a HIP call failed or d_comp_bytes is too small, -7 no range left.
 *                     After an error every further call fails the same way; the handle is still to be closed
 *   svx_stage_tables  the last group's blocks: payload offset in d_comp, payload bytes, ISIZE, file offset; cap >= their number
 *   svx_stage_close   from any state: the pool is joined, the descriptor closed, the events destroyed.  The copies that are
 *                     enqueued are the caller's to wait for (its stream) before it reuses the slots */
void*          svx_stage_open(const char* path, int threads, const uint64_t* ranges, int n_ranges, const uint64_t* slot_ptrs, int n_slots,
                              uint64_t slot_bytes, int device, void* copy_stream);
int64_t        svx_stage_group(void* stage, uint8_t* d_comp, uint64_t d_comp_bytes, uint64_t* used, double* waits, double* stamps,
                               uint64_t stamps_cap);
int            svx_stage_tables(void* stage, uint64_t* src_off, uint32_t* src_len, uint32_t* isize, uint64_t* coff, uint64_t cap);
void           svx_stage_close(void* stage);

/* Streaming ingestion, one reference sequence at a time (replaces the reference's window-by-window
 * AlignmentFile.fetch(chrom, start, end), run_collection.py:23-26, by one pass over the file that hands chromosome k
 * to the caller while chromosome k+1 is being read and inflated on the handle's own threads):
 *   svx_bam_stream_open  -> opaque stream or NULL (svx_bam_error()); voffs = n_ranges pairs of BGZF virtual offsets
 *                           from the .bai (a rank's chromosomes, ascending), n_ranges = 0: every record of the file;
 *                           threads <= 0: the CPUs of the process (max 128); flags as svx_bam_open
 *   svx_bam_stream_next  -> the next reference's records as a handle for svx_bam_sizes / svx_bam_export /
 *                           svx_bam_seq / svx_bam_close (QNAME ids count from 0 in every part), or NULL with
 *                           *status = 0 at the end, -1 on error; blocks while that part is being decoded
 *   svx_bam_stream_close -> stops the threads, frees what was not handed out */
void*          svx_bam_stream_open(const char* path, int threads, int flags, const uint64_t* voffs, int n_ranges);
void*          svx_bam_stream_next(void* stream, int* status);
void           svx_bam_stream_close(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVX_H */
