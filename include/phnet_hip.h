/* C-ABI of libphnet_hip.so: the MI355X (gfx950) kernels behind PHNet's per-clip hot path.
 *
 * This is the drop-in boundary (DESIGN.md "Boundary"): plain pointers and sizes, no torch types.
 * The only native FFI the reference has on this path is the pybind11 module nms_impl
 * (libs/ops/csrc/nms.cpp:44-61 -> nms_kernel.cu:147-192); phnet_lane_nms replaces it.  Every other entry
 * point replaces an ATen/cuDNN/cuBLAS call the reference's Python makes (file:line given per function) and
 * follows the same conventions:
 *   - all pointers are DEVICE pointers (hipMalloc / torch.cuda memory), fp32 unless stated otherwise;
 *   - outputs and workspaces are CALLER-allocated; nothing here allocates, frees or synchronises;
 *   - `stream` is a hipStream_t (NULL = the legacy default stream); kernels are enqueued, not awaited;
 *   - return value: 0 = enqueued, <0 = error (no work enqueued unless stated):
 *       PHNET_ERR_ARG (-1) bad shape / null pointer / unsupported size,
 *       PHNET_ERR_WORKSPACE (-2) workspace too small, PHNET_ERR_LAUNCH (-3) HIP launch error;
 *   - re-entrant, with one exception: the conv / Linear / gate / dynamic-head entries read the process-global tuning struct
 *     (kernel A/B switches; defaults = the product path).  Only include/phnet_hip_tuning.h writes it, and it must not change
 *     while a step is being captured into a hipGraph.
 * Activation layout is NHWC; convolution weights are OHWI ([Co][R][S][Ci]) = the memory order of a
 * torch.channels_last OIHW parameter, so reference checkpoints load without a re-layout pass.
 */
#ifndef PHNET_HIP_H
#define PHNET_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PHNET_OK 0
#define PHNET_ERR_ARG (-1)
#define PHNET_ERR_WORKSPACE (-2)
#define PHNET_ERR_LAUNCH (-3)
#define PHNET_ABI_VERSION 1

int phnet_abi_version(void);

/* ---- lane NMS: replaces nms_impl.nms_forward (libs/ops/csrc/nms.cpp:44-57, nms_kernel.cu:26-192) ----
 * rows   [frames][k_max][5+n_offsets]  (cls0, cls1, start_y, start_x_px, length_strips, x_0.. px)
 * scores [frames][k_max];  counts [frames] int32 valid rows per frame, or NULL (= k_max for every frame)
 * keep [frames][k_max] int64 (first num entries valid, rest 0), num_to_keep [frames] int64,
 * parent [frames][k_max] int64 (1-based group id, 0 = none).  Score ties are broken by lower row index.
 * Limits: k_max <= ~900 (single-workgroup design), n_offsets <= 250. */
int phnet_lane_nms(const float* rows, const float* scores, const int32_t* counts, int64_t frames,
                   int64_t k_max, int32_t n_offsets, float thresh, int64_t top_k,
                   int64_t* keep, int64_t* num_to_keep, int64_t* parent, void* stream);

/* ---- fused eval decode: replaces DetNetV2.get_lanes up to the kept rows (libs/models/Router4OL.py:441-471: softmax +
 * confidence mask + boolean-mask compaction + NMS rows + libs.ops.nms + keep[:num] + gather + length rounding) in one
 * launch without host synchronisation.  lines [frames][N][6+S], N <= 256, top_k <= 64.  keep_mask u8 [frames][N];
 * num i64 [frames]; keep_c i64 [frames][top_k] (indices into the compacted candidate list, NMS order, -1 padded = the
 * reference's `keep`); anchors / anchors_sorted i64 [frames][top_k] (anchor indices, NMS order / ascending);
 * kept_rows [frames][top_k][6+S] (column 5 rounded to strips; zero rows beyond num). */
int phnet_lane_decode(const float* lines, int64_t frames, int32_t N, int32_t n_offsets, float conf_thresh,
                      float nms_thresh, int64_t top_k, float img_w, uint8_t* keep_mask, int64_t* num,
                      int64_t* keep_c, int64_t* anchors, int64_t* anchors_sorted, float* kept_rows, void* stream);

/* ---- lane polylines: replaces DetNetV2.predictions_to_pred (libs/models/Router4OL.py:394-435) up to the points of each lane,
 * one launch for all frames, no host synchronisation (csrc/lane_points.hip; the rules are listed there and in DESIGN.md
 * "Streaming path").  kept_rows [F][L][6+S] and num i64 [F] as phnet_lane_decode writes them (column 5 in strips); prior_ys [S].
 * points [F][L][S][2]: the (x, y) pairs of the frame's lanes, normalised, in the host's order (descending offset index); lanes
 *   are PACKED - lane k is the k-th lane the host list would hold; the unused tail of a lane and unused lanes are zeros.
 * count i32 [F][L]: points of packed lane k (0 = unused);  lanes_num i32 [F]: kept slots that yield more than one point;
 * slot i32 [F][L]: the kept_rows slot packed lane k came from (-1 = unused) - conf, start_y, start_x are columns 1, 2, 3 of it.
 * Values are copied, never computed: bit-identical to the host's float64 points after widening.  A row whose start_y or
 * length is NaN or +-inf (the host code raises on it) is not a lane.  Every output element is written on every call.
 * Limits: 1 <= F < 2^31, 1 <= L <= 64, 2 <= S <= 256. */
int phnet_lane_points(const float* kept_rows, const int64_t* num, const float* prior_ys, int64_t F, int32_t L, int32_t S,
                      float* points, int32_t* count, int32_t* lanes_num, int32_t* slot, void* stream);

/* ---- lane identities: a stable id per lane across the frames of a stream (csrc/lane_track.hip; no counterpart in the reference,
 * which leaves an unordered lane set per frame).  One launch for B streams, one wavefront per stream walking its T frames in order
 * (T = 1: the streaming step; T > 1: a clip), no host synchronisation.  kept_rows [B][T][L][6+S] and num i64 [B][T] as
 * phnet_lane_decode writes them.  State, read and written by the call (caller-owned, one set per B streams): trk_id i32 [B][M]
 * (0 = free slot), trk_missed i32 [B][M], trk_hits i32 [B][M], trk_ext i32 [B][M][2] (start, end), trk_x [B][M][S] (the xs of the
 * last matched row: copied, never computed), next_id i32 [B] (starts at 1; < 1 is read as 1).  Out, every element written on every
 * call: track_id i32 [B][T][L] (-1 = not trackable), track_hits i32 [B][T][L] (0 = not trackable).
 * Per frame, in this order (a slot is live when its id != 0):
 *   1. start = clamp(rint(double(r[2]) * (S-1)), 0, S-1), end = min(start + rint(double(r[5])) - 1, S-1) (the extent rule of
 *      phnet_lane_points).  Row d is trackable iff d < clamp(num, 0, L), r[2] and r[5] are finite and end >= start; any other row
 *      gets track_id -1, hits 0 and never touches the state.
 *   2. (trackable row d, live slot k): lo = max(starts), hi = min(ends), skipped if hi < lo; sum = f32 accumulation of
 *      |row_x[i] - slot_x[i]| for i = lo..hi ascending, each term a < b ? b - a : a - b, not contracted; cnt = hi - lo + 1.  The
 *      pair is a candidate iff sum < thr * (float)cnt (one f32 multiply, strict <; a NaN in the range: not a candidate).
 *   3. greedy, smallest mean first: (sum_p, cnt_p) before (sum_q, cnt_q) iff double(sum_p) * cnt_q < double(sum_q) * cnt_p (exact,
 *      no division), ties to the lower d, then the lower k; pairs are taken in that order, skipping rows and slots already taken.
 *      A match copies the row's xs and extent into the slot, missed = 0, hits += 1; the row gets the slot's id and hits.
 *   4. every live slot not matched: missed += 1; missed > max_age frees it (id = 0).
 *   5. every trackable unmatched row, ascending d: the lowest free slot, else the slot with the largest missed among those neither
 *      matched nor filled in this frame (ties: lowest slot); id = next_id, next_id advances and wraps from 2^31 - 1 to 1;
 *      hits = 1, missed = 0, the row is copied in.
 * thr is in the units of kept_rows (xs normalised by img_w - 1).  A reset of a stream is trk_id[b][*] = 0 by the caller; next_id is
 * kept, so ids never repeat within a stream's state.
 * Limits (PHNET_ERR_ARG before any launch): 1 <= L <= M <= 64, 2 <= S <= 256, (L + M) * S + 2 * L * M <= 15360 (the LDS staging),
 * 1 <= T, 1 <= B < 2^31, max_age >= 0, thr finite and > 0, all pointers non-null. */
int phnet_lane_track(const float* kept_rows, const int64_t* num, int64_t B, int32_t T, int32_t L, int32_t S, int32_t M, float thr,
                     int32_t max_age, int32_t* trk_id, int32_t* trk_missed, int32_t* trk_hits, int32_t* trk_ext, float* trk_x,
                     int32_t* next_id, int32_t* track_id, int32_t* track_hits, void* stream);

/* ---- lane overlay: the polylines of phnet_lane_points back on a picture (csrc/lane_draw.hip; replaces the host loops of the
 * reference's test script, testOL.py:165-227 predlanesV2 / generate_seg_from_line - int() of every point, cv2.line(thickness = 12)
 * lane by lane - and the 50/50 blend of libs/utils/utility.py:66-68).  One launch for F frames, no host synchronisation, no
 * atomics; every element of every requested output is written exactly once on every call, so nothing has to be cleared.
 * points f32 [F][L][S][2] (8-byte aligned), count i32 [F][L] (clamped to [0, S]), lanes_num i32 [F] (clamped to [0, L]) as
 * phnet_lane_points writes them.  slot i32 [F][L] (phnet_lane_points) with track_id i32 [F][L] (phnet_lane_track): optional, colour
 * by identity; slot alone is ignored.  Outputs, either or both: label_map u8 [F][out_h][out_w]; overlay u8 [F][out_h][out_w][3]
 * packed RGB.  src (optional, read for the overlay only): F frames of out_h x out_w pixels, frame_stride bytes apart; src_format
 * 0 = none, 1 = packed RGB rows of `pitch` >= 3 out_w bytes, 2 = NV12, 3 = YUYV - for 2 and 3 pitch, chroma_offset and csc_host [10]
 * (HOST pointer) mean what they mean to phnet_preprocess_yuv with H0 = out_h, W0 = out_w.  palette u8 [256][3] on the device
 * (needed with `overlay`); alpha 0..256.
 *   1. point to pixel: px = trunc(double(x) * sx), py = trunc(double(y) * sy + oy) - float64, product and sum rounded separately,
 *      truncation toward zero: Python's int() on the float64 expression (testOL.py:171).  sx = src_w, sy = src_h - crop, oy = crop
 *      is the reference's mapping.  A point with x <= 0 or y <= 0 is skipped (testOL.py:169); so is a point that is NaN or +-inf or
 *      whose px or py lies outside [-8192, 8192].  Consecutive surviving points of a lane form its segments; a lane with fewer than
 *      2 survivors draws nothing.
 *   2. coverage: pixel (u, v) belongs to a segment (x0, y0)-(x1, y1) iff, with q = (u - x0, v - y0), d = (x1 - x0, y1 - y0),
 *      L2 = d.d, w = lane_width:  q.d <= 0: 4 q.q <= w^2;  q.d >= L2: 4 |(u - x1, v - y1)|^2 <= w^2;  else 4 (qx dy - qy dx)^2 <=
 *      w^2 L2 - exact integers, the test of oracle/culane_cpu.py raster_lane and phnet_lane_raster, so a map agrees with what the
 *      evaluator counts.  The pixel grid is the only clipping.  PARITY UNPINNED against cv2.line's scan conversion.
 *   3. order: among the lanes covering a pixel the one with the highest packed index k wins (the painter's order of the
 *      reference's loop, testOL.py:174-177).
 *   4. value of lane k: without track_id v = k + 1.  With it id = track_id[f][slot[f][k]] (a slot outside [0, L) counts as id 0):
 *      v = 1 + (id - 1) mod 254 for id >= 1, v = 255 for id <= 0 (a lane without an identity).  v = 0 is background.  The label map
 *      stores v.
 *   5. overlay: the source pixel as 8-bit RGB - NV12 / YUYV through the integer conversion of phnet_preprocess_yuv, chroma
 *      replicated; without a source black.  v = 0: the source pixel.  Else out_c = (src_c (256 - alpha) + palette[v][c] alpha + 128)
 *      >> 8: alpha = 256 is cv2.line onto the frame, alpha = 128 addWeighted(0.5, 0.5).
 * A frame with lanes_num = 0 gives a zero map and an overlay equal to the converted source.
 * PHNET_ERR_ARG before any launch: null points / count / lanes_num, points not 8-byte aligned, track_id without slot, no output,
 * overlay without palette, F < 1 or F * ceil(out_w / 128) * ceil(out_h / 8) >= 2^31, L outside 1 <= L <= 64 or S outside
 * 2 <= S <= 256, non-finite sx / sy / oy, out_h or out_w outside 1..4096, lane_width outside 1..256, alpha outside 0..256, an unknown
 * src_format; with a source: null src, odd out_w (NV12, YUYV) or odd out_h (NV12), pitch or chroma_offset too small, frame_stride
 * smaller than the bytes a frame spans, a frame that spans >= 2^31 bytes, a null or out-of-bound colour matrix (NV12, YUYV). */
int phnet_lane_draw(const float* points, const int32_t* count, const int32_t* lanes_num, const int32_t* slot,
                    const int32_t* track_id, int64_t F, int32_t L, int32_t S, double sx, double sy, double oy,
                    int32_t out_h, int32_t out_w, int32_t lane_width, const uint8_t* src, int32_t src_format,
                    int64_t frame_stride, int32_t pitch, int64_t chroma_offset, const int32_t* csc_host,
                    const uint8_t* palette, int32_t alpha, uint8_t* label_map, uint8_t* overlay, void* stream);

/* ---- training targets: annotated lane points -> the label rows the criterion consumes (csrc/lane_targets.hip; replaces the label
 * half of the reference's per-frame pipeline: datasetOL.py:47-59 crop / flip, transforms.py:251-347 transform_annotation,
 * filter_lane, sample_lane).  One launch for F frames, one wavefront per (frame, output row), no host synchronisation.
 * points f32 [F][Lin][P][2] (x, y), counts i32 [F][Lin] (clamped to [0, P]), lanes_num i32 [F] (clamped to [0, Lin]); entries
 * beyond a count are never read.  offsets_ys f64 [S] on the device: the reference's np.arange(img_h, -1, -strip_size), strictly
 * descending, taken as numpy builds it (its last entry is not exactly 0).  out f32 [F][R][6+S], every element written on every
 * call.  Float64 throughout (input points widened exactly), nothing contracted, one cast to float32 at the end.
 * Per frame:
 *   0. map, per point: y = y - crop; flip: x = (src_w - 1) - x; x = x * scale_x; y = y * scale_y.
 *   1. lanes with more than 2 points survive and are numbered in order; number r owns row r; numbers >= R are ignored.
 *   2. default row: [0] = 1, [1] = 0, the rest -1e5.  Rows without a lane, and lanes with a non-finite mapped coordinate, keep it.
 *   3. stable sort by descending y; of equal y the first in input order stays; x = (x * img_w) / img_w, y = (y * img_h) / img_h.
 *      n points remain; n < 2 keeps the default row.
 *   4. interpolant over ascending y: n = 2 the line, n = 3 the parabola (Newton form), n >= 4 the not-a-knot cubic spline (knot
 *      derivatives by a tridiagonal solve without pivoting; Horner evaluation in the interval found by binary search).
 *   5. table order: ys > y_max: the line through the two bottom-most points; y_min <= ys <= y_max: the interpolant; ys < y_min:
 *      dropped.  No row of the second kind keeps the default row.
 *   6. inside iff 0 <= x < img_w.  All outside values come first, then the inside ones, each in table order.
 *   7. n_in <= 1 keeps the default row.  Else [0] = 0, [1] = 1, [2] = n_out / (S-1), [3] = inside[0] / (img_w - 1), [4] = mean over
 *      i = 1..n_in-1 of t_i = atan(i * strip_size / (inside[i] - inside[0] + 1e-5)) / pi (1 - |t_i| where not t_i > 0), summed in
 *      ascending i, [5] = n_in / (S-1), [6..] = the values of rule 6, then -1e5.
 * Limits (PHNET_ERR_ARG before any launch): 1 <= F < 2^31, 1 <= Lin <= 64, 2 <= P <= 256, 1 <= R <= 64, 2 <= S <= 256; img_h,
 * img_w, strip_size, scale_x, scale_y finite and > 0; crop and src_w finite; flip 0 or 1; all pointers non-null. */
int phnet_lane_targets(const float* points, const int32_t* counts, const int32_t* lanes_num, const double* offsets_ys, float* out,
                       int64_t F, int32_t Lin, int32_t P, int32_t R, int32_t S, double img_h, double img_w, double strip_size,
                       double crop, double src_w, double scale_x, double scale_y, int32_t flip, void* stream);
/* The same launch behind an augmented image (phnet_augment_u8 below): one rule more, after rule 0, in output pixels:
 *   0b. flip2[f] != 0: x = (img_w - 1) - x; then (x, y) = ((f00 x + f01 y) + f02, (f10 x + f11 y) + f12), f = fwd[f] - float64, not
 *       contracted.  Everything from rule 1 on is unchanged: a lane that the rotation makes non-monotonic in y goes through the sort
 *       and the de-duplication of rule 3, a non-finite product keeps the default row (rule 2).
 * flip2 i32 [F], fwd f64 [F][6] (the source -> output matrix, row-major 2 x 3: the inverse of the image's matrix), on the device;
 * either may be null and its step is skipped: with both null this is phnet_lane_targets, bit for bit.  Limits as above. */
int phnet_lane_targets_aug(const float* points, const int32_t* counts, const int32_t* lanes_num, const double* offsets_ys, float* out,
                           int64_t F, int32_t Lin, int32_t P, int32_t R, int32_t S, double img_h, double img_w, double strip_size,
                           double crop, double src_w, double scale_x, double scale_y, int32_t flip, const int32_t* flip2,
                           const double* fwd, void* stream);
/* The same launch with the reference's clip_out_of_image_() (transforms.py:68) between the map and the filter, and the number of
 * fragments it leaves per frame.  One rule more, on the mapped points in INPUT order, after rules 0 / 0b and before rule 1, in
 * float64, not contracted:
 *   0c. (clip = 1) rectangle: Wc = img_w - 1e-3, Hc = img_h - 1e-3; a point is in iff 0 <= x <= Wc and 0 <= y <= Hc (false for NaN).
 *       A lane with a non-finite mapped coordinate is not clipped: it is ONE fragment with all its points (rule 2 keeps its row the
 *       default row, as before).  For a finite lane of n points every maximal run of consecutive in-points p_a .. p_b gives one
 *       fragment [E] p_a .. p_b [X]: E exists iff a > 0 and is the crossing of the segment p_a -> p_(a-1); X exists iff b < n - 1 and
 *       is the crossing of p_b -> p_(b+1).  A crossing is computed from the in endpoint q towards the out endpoint o: for each
 *       coordinate c whose bound o violates (the bound is 0, Wc or Hc), t_c = (bound - q_c) / (o_c - q_c); t is the smaller of the
 *       two, an unviolated coordinate does not take part; the point is q + t * (o - q), and the coordinate(s) that gave t are set
 *       to the bound itself (on a tie both: a corner).  A crossing equal to q in both coordinates is dropped.  A segment with
 *       BOTH ends out is never clipped, even where it crosses the image: its two-point fragment would fall to rule 1, so it is not
 *       produced.
 *   1 on fragments: fragments of more than 2 points survive and are numbered in order of (input lane, run); number r owns row r;
 *       numbers >= R are ignored.  Everything from rule 2 on is unchanged, with the fragment's points [E] p_a .. p_b [X] in that
 *       order as the lane's input order.
 * A frame with no point outside the rectangle encodes exactly as without the rule; with clip = 0 this is phnet_lane_targets_aug, bit
 * for bit.  frag_count i32 [F] on the device, or null: the surviving fragments of the frame BEFORE the R cap (with clip = 0: the
 * surviving lanes), written on every call.  flip2 and fwd as above.  Limits as above, and clip 0 or 1, and 2 <= P <= 254 with
 * clip = 1 (a fragment has up to P + 2 points, and the staging holds 256). */
int phnet_lane_targets_clip(const float* points, const int32_t* counts, const int32_t* lanes_num, const double* offsets_ys, float* out,
                            int64_t F, int32_t Lin, int32_t P, int32_t R, int32_t S, double img_h, double img_w, double strip_size,
                            double crop, double src_w, double scale_x, double scale_y, int32_t flip, const int32_t* flip2,
                            const double* fwd, int32_t clip, int32_t* frag_count, void* stream);

/* ---- lane-anchor ROI pooling: replaces F.grid_sample(..., align_corners=True) + permutes
 * (libs/models/Router4OL.py:132-150, 269-272) and its backward (ATen grid_sampler_2d_backward).
 * fmap [B][h][w][64]; xs [B][N][P] = priors_on_featmap (un-flipped); ys [P] = prior_feat_ys; out [B][N][P][64]. */
/* out_cp (optional): the same samples laid out [B][N][64][P] for the routing gate. */
int phnet_roi_pool_fwd(const float* fmap, const float* xs, const float* ys, float* out, float* out_cp,
                       int32_t B, int32_t N, int32_t P, int32_t h, int32_t w, int32_t C, void* stream);
/* dmap [B][h][w][64] is accumulated into (may be NULL); dxs [B][N][P] is overwritten (may be NULL). */
int phnet_roi_pool_bwd(const float* dout, const float* fmap, const float* xs, const float* ys,
                       float* dmap, float* dxs,
                       int32_t B, int32_t N, int32_t P, int32_t h, int32_t w, int32_t C, void* stream);

/* ---- convolution / linear on fp32 MFMA: replaces F.conv2d (libs/models/resnet.py:79-95,293-307;
 * libs/models/fpn.py:109-163) and F.linear (Router4OL.py:308-392, utils/dynamic_head.py:31-59, Router.py:72-81).
 * x [N][Hi][Wi][Ci], w [Co][R][S][Ci], bias [Co] or NULL, y [N][Ho][Wo][Co]; Ci%4==0, Co%4==0.
 * workspace optional (split-K partial sums; the plan splits only as far as ws_bytes holds splits * N*Ho*Wo*Co*4.  What
 * phnet_amd.hip_ops.splitk_workspace_bytes hands every launch: 8 slabs of the output where it has fewer than 2^23 elements, else none).
 * A Linear layer ([M][1][1][K] image, 1x1 filter) of many rows runs on the tall tiles of csrc/linrows.hip where that is faster, same bits. */
int phnet_conv2d_fwd(const float* x, const float* w, const float* bias, float* y,
                     int32_t N, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co, int32_t R, int32_t S,
                     int32_t stride, int32_t pad, int32_t relu, void* workspace, uint64_t ws_bytes, void* stream);
/* forward with a fused epilogue: y = relu?(conv + bias + addend) (addend shaped like y: the residual branch of an eval-mode
 * BatchNorm block whose scale / shift were folded into w / bias), and / or stats = per-channel (sum | sum of squares) partials
 * of y for a following training-mode BatchNorm: phnet_conv2d_stats_blocks() rows of 2*Co floats, consumed by
 * phnet_bn_finalize_partials (no separate statistics pass over y; needs bias == addend == NULL, relu == 0, Co = 2^k <= 1024). */
uint64_t phnet_conv2d_stats_blocks(int64_t M, int32_t Co, int32_t K, uint64_t ws_bytes);
int phnet_conv2d_fwd_fused(const float* x, const float* w, const float* bias, const float* addend, float* y, float* stats,
                           int32_t N, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co, int32_t R, int32_t S,
                           int32_t stride, int32_t pad, int32_t relu, void* workspace, uint64_t ws_bytes, void* stream);
/* dx = dgrad(dy, w) (+ addend): addend is optional, shaped like dx, and may alias dx. */
int phnet_conv2d_dgrad(const float* dy, const float* w, const float* addend, float* dx,
                       int32_t N, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co, int32_t R, int32_t S,
                       int32_t stride, int32_t pad, void* workspace, uint64_t ws_bytes, void* stream);
/* ---- 3x3 / stride 1 / pad 1 convolutions on PACKED weights (csrc/conv3p.hip): the trunk / FPN 3x3 layers of
 * libs/models/resnet.py:79-95 and fpn.py:156-160, forward and data gradient.  phnet_conv3p_pack splits a weight
 * [Co][3][3][Ci] once into its three bf16 terms, laid out in MFMA fragment order (dgrad = 0: the forward's operand;
 * 1: the data gradient's - flipped taps, transposed channels); phnet_conv3p_fwd then computes
 *   y = conv3x3(x, w) (+ bias) (+ addend) (ReLU)          on the dgrad = 0 packing (Ca = Ci, Nn = Co), or
 *   dx = conv3x3_dgrad(dy, w) (+ addend)                   on the dgrad = 1 packing (x = dy, Ca = Co, Nn = Ci),
 * same arithmetic and epilogues as phnet_conv2d_fwd_fused (stats: rows of 2*Nn floats, phnet_conv3p_stats_blocks of them).
 * Needs Ca % 16 == 0, Nn % 64 == 0 (phnet_conv3p_applies). */
int phnet_conv3p_applies(int64_t M, int32_t Ca, int32_t Nn);
uint64_t phnet_conv3p_packed_bytes(int32_t Co, int32_t Ci);
int phnet_conv3p_pack(const float* w, void* packed, int32_t Co, int32_t Ci, int32_t dgrad, void* stream);
/* all 3x3 weights of a model in one launch: jobs = DEVICE array of njobs records {const float* w; void* dst; int32 Co, Ci, dgrad, 0;
 * int64 first} sorted by `first` = running sum of the jobs' item counts 9*(Ca/16)*(Nn/32)*64; total = the sum of all counts */
int phnet_conv3p_pack_jobs(const void* jobs, int32_t njobs, int64_t total, void* stream);
/* The one-plane image of the bf16 inference arithmetic (phnet_tune_mma(4), include/phnet_hip_tuning.h): every weight rounded to
 * bf16 once, same fragment order, exactly a third of phnet_conv3p_packed_bytes; forward packing only (job records with dgrad = 0).
 * While mode 4 is set, phnet_conv3p_fwd takes THIS image (and the three-plane one in every other mode): the caller keeps the
 * image and the mode of the launch together. */
uint64_t phnet_conv3p_packed_bytes_bf16(int32_t Co, int32_t Ci);
int phnet_conv3p_pack_bf16(const float* w, void* packed, int32_t Co, int32_t Ci, void* stream);
int phnet_conv3p_pack_jobs_bf16(const void* jobs, int32_t njobs, int64_t total, void* stream);
uint64_t phnet_conv3p_stats_blocks(int64_t M, int32_t Ca, int32_t Nn, uint64_t ws_bytes);
int phnet_conv3p_fwd(const float* x, const void* packed, const float* bias, const float* addend, float* y, float* stats,
                     int32_t N, int32_t H, int32_t W, int32_t Ca, int32_t Nn, int32_t relu,
                     void* workspace, uint64_t ws_bytes, void* stream);
/* host-side queries (no device work, callable without a GPU; HOST pointers), answered by the decision functions the launches
 * call.  phnet_conv2d_plan: tile, split-K factor and K-tile depth of a forward GEMM of M x Co x K (M < 2^31).  phnet_*_kernel:
 * the instantiation the launch entry of the same shape arguments runs, as rocprofv3 spells it after the namespace (e.g.
 * "conv_igemm_kernel<64, 64, false, 16, true, 3, 4, true>"; name_cap bytes), and its split factor.  phnet_conv2d_kernel:
 * dgrad = 0 names phnet_conv2d_fwd / _fwd_fused, 1 phnet_conv2d_dgrad; ws_bytes = 0 = no workspace.  It names the launch WITHOUT
 * addend and stats: a Linear layer that has one runs conv_igemm_kernel where the query says linrows_kernel (the only difference). */
int phnet_conv2d_plan(int64_t M, int32_t Co, int32_t K, uint64_t ws_bytes, int32_t* bm, int32_t* bn, int32_t* splits,
                      int32_t* k_tile);
int phnet_conv2d_kernel(int32_t dgrad, int32_t N, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co, int32_t R, int32_t S,
                        int32_t stride, int32_t pad, uint64_t ws_bytes, char* name, int32_t name_cap, int32_t* splits);
int phnet_conv2d_wgrad_kernel(int32_t N, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co, int32_t R, int32_t S, int32_t stride,
                              int32_t pad, int32_t has_dbias, uint64_t ws_bytes, char* name, int32_t name_cap, int32_t* splits);
int phnet_linear_bwd_kernel(int32_t M, int32_t K, int32_t N, int32_t has_relu_mask, char* name, int32_t name_cap);
int phnet_conv3p_kernel(int64_t M, int32_t Ca, int32_t Nn, uint64_t ws_bytes, char* name, int32_t name_cap, int32_t* splits);
uint64_t phnet_conv2d_wgrad_workspace(int32_t N, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co,
                                      int32_t R, int32_t S, int32_t stride, int32_t pad);
/* dbias (optional, [Co]) = sum of dy over all pixels = the bias gradient, produced by the same launch. */
int phnet_conv2d_wgrad(const float* dy, const float* x, float* dw, float* dbias,
                       int32_t N, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co, int32_t R, int32_t S,
                       int32_t stride, int32_t pad, int32_t accumulate, void* workspace, uint64_t ws_bytes, void* stream);
/* Backward of a Linear layer over few rows (the M = 240 layers of the lane head) as ONE launch: dx [M][K] = dy w and
 * dw [N][K] (+)= dy^T x, dbias [N] (+)= column sums of dy (dbias optional).  dy [M][N], x [M][K], w [N][K] row-major.
 * phnet_linear_bwd_fusable tells whether a shape qualifies (M <= 256, N <= 640, few tiles); otherwise use
 * phnet_conv2d_dgrad + phnet_conv2d_wgrad. */
int phnet_linear_bwd_fusable(int64_t M, int64_t K, int64_t N);
int phnet_linear_bwd(const float* dy, const float* x, const float* w, const float* relu_y, float* dx, float* dw, float* dbias,
                     int32_t M, int32_t K, int32_t N, int32_t accumulate, void* stream);   /* relu_y (optional, [M][N]): saved
                     output of a layer that ended in a ReLU; dy is masked by relu_y > 0 while it is staged */
/* stem helpers: NCHW 3-channel frames -> NHWC padded to 4 channels; innermost-dimension pad/truncate. */
int phnet_nchw3_to_nhwc4(const float* x, float* y, int32_t N, int32_t H, int32_t W, void* stream);
int phnet_pad_channels(const float* src, float* dst, int64_t rows, int32_t cs, int32_t cd, void* stream);

/* ---- one-shot all-reduce of small messages over peer-mapped buffers (csrc/ipc_allreduce.hip): the SyncBatchNorm statistic
 * exchanges of trainOL.py:141 (<= 8 KB, 72 per step, on the critical path).  Each rank allocates an exchange buffer
 * (phnet_ipc_alloc, phnet_ipc_buffer_bytes), hands its 64-byte handle to the peers over any host channel, maps theirs
 * (phnet_ipc_open_handle) and passes the table of mapped pointers (a DEVICE array, entry `rank` = the local buffer) to
 * phnet_oneshot_allreduce: in place, SUM, contributions added in rank order (bit-identical on every rank), one launch on
 * `stream`, capturable.  ctrl: DEVICE {uint32 sequence, uint32 error}, sequence initialised to 1 on every rank. */
uint64_t phnet_ipc_buffer_bytes(int32_t world, uint64_t max_bytes);
int phnet_ipc_alloc(uint64_t bytes, void** ptr);
int phnet_ipc_free(void* ptr);
int phnet_ipc_get_handle(void* ptr, void* handle64);
int phnet_ipc_open_handle(const void* handle64, void** ptr);
int phnet_ipc_close_handle(void* ptr);
int phnet_oneshot_allreduce(void* data, int32_t count, int32_t dtype, const void* peers, int32_t rank, int32_t world,
                            int32_t cap, void* ctrl, void* stream);

/* ---- BatchNorm2d / ReLU / residual: replaces F.batch_norm + relu + add (libs/models/resnet.py:79-95, 293-297) ---- */
uint64_t phnet_channel_partials_size(int64_t M, int32_t C);   /* floats needed in `partial` */
int phnet_bn_fwd_stats(const float* x, int64_t M, int32_t C, float eps, float momentum,
                       const float* gamma, const float* beta, float* running_mean, float* running_var,
                       float* save_mean, float* save_invstd, float* scale, float* shift,
                       float* partial, int32_t training, void* stream);
/* the finalize half of phnet_bn_fwd_stats on partials somebody else produced (phnet_conv2d_fwd_fused): partial [nblk][2C] */
int phnet_bn_finalize_partials(const float* partial, int64_t nblk, int64_t M, int32_t C, float eps, float momentum,
                               const float* gamma, const float* beta, float* running_mean, float* running_var,
                               float* save_mean, float* save_invstd, float* scale, float* shift, void* stream);
int phnet_bn_apply(const float* x, const float* scale, const float* shift, const float* residual, float* y,
                   int64_t M, int32_t C, int32_t relu, void* stream);
int phnet_bn_bwd(const float* dy, const float* x, const float* y, const float* save_mean,
                 const float* save_invstd, const float* gamma, float* dx, float* dres,
                 float* dgamma, float* dbeta, float* partial, float* c1, float* c2,
                 int64_t M, int32_t C, int32_t relu, int32_t dres_accumulate, int32_t param_accumulate, void* stream);

/* split form for SyncBatchNorm (trainOL.py:141): local sums[2][C] = (sum g*xhat, sum g) -> caller all-reduces -> apply. */
int phnet_bn_bwd_reduce(const float* dy, const float* x, const float* y, const float* mean, const float* invstd,
                        float* sums, float* partial, float* c1_scratch, float* c2_scratch,
                        int64_t M, int32_t C, int32_t relu, void* stream);
int phnet_bn_bwd_apply(const float* dy, const float* x, const float* y, const float* mean, const float* invstd,
                       const float* gamma, const float* c1, const float* c2, float* dx, float* dres,
                       int64_t M, int32_t C, int32_t relu, int32_t dres_accumulate, void* stream);

/* device-resident SyncBatchNorm (trainOL.py:141): no host read of the element count, so the step stays sync-free.
 * fwd: phnet_bn_local_sums -> all-reduce(SUM) sums[2C+1] (fp64: sum x, sum x^2, count) -> phnet_bn_finalize_sums -> phnet_bn_apply
 * bwd: phnet_bn_bwd_reduce -> all-reduce(SUM) sums[2][C] -> phnet_bn_bwd_apply_sums (count = &sums_fwd[2C]) */
int phnet_bn_local_sums(const float* x, int64_t M, int32_t C, float* partial, double* sums, void* stream);
/* the same sums from the per-block partials of the convolution's epilogue (phnet_conv2d_fwd_fused stats): no pass over x */
int phnet_bn_partials_to_sums(const float* partial, int64_t nblk, int64_t M, int32_t C, double* sums, void* stream);
int phnet_bn_finalize_sums(const double* sums, int32_t C, float eps, float momentum, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                           float* scale, float* shift, void* stream);
int phnet_bn_bwd_apply_sums(const float* dy, const float* x, const float* y, const float* mean, const float* invstd,
                            const float* gamma, const float* sums, const double* count, float* c1, float* c2,
                            float* dx, float* dres, int64_t M, int32_t C, int32_t relu, int32_t dres_accumulate, void* stream);

/* ---- input pre-processing of a clip: libs/dataset/openlane/datasetOL.py:40-52 (crop top rows, optional
 * flip), transforms.py:150-156 (iaa.Resize = cv2 INTER_CUBIC on uint8), datasetOL.py:63-75,11-17 (ToTensor, Normalize, stack).
 * frames u8 [T][H0][W0][3] RGB on the device; out f32 NCHW [T][3][oh][ow] (layout 0) or NHWC4 [T][oh][ow][4] (layout 1);
 * out_u8 optional [T][oh][ow][3]; xi/xc [ow][4], yi/yc [oh][4]: clamped source indices (int32) and 11-bit taps (int16, each saturate_cast<short>(c * 2048): sum 2047..2049)
 * of the half-pixel a = -0.75 cubic kernel, built once per geometry by the caller; mean3 / std3 are HOST pointers. ---- */
int phnet_preprocess_u8(const uint8_t* frames, float* out, uint8_t* out_u8,
                        const int32_t* xi, const int16_t* xc, const int32_t* yi, const int16_t* yc,
                        int32_t T, int32_t H0, int32_t W0, int32_t crop_top, int32_t out_h, int32_t out_w, int32_t flip,
                        int32_t layout, const float* mean3_host, const float* std3_host, void* stream);
/* The same launch on camera surfaces (no RGB image in memory).  frames: T surfaces frame_stride bytes apart.  format 0 = NV12:
 * H0 luma rows of `pitch` bytes, then from byte chroma_offset (>= pitch * H0) on H0/2 rows of interleaved U,V, `pitch` bytes
 * each; format 1 = YUYV: H0 rows of `pitch` bytes Y0 U Y1 V (chroma_offset ignored).  pitch >= W0 (NV12) / 2 W0 (YUYV).
 * Colour of source pixel (r, x), r counted in the UNCROPPED frame, in int32:
 *   c = clamp((m[c][0] (Y - y0) + m[c][1] (U - 128) + m[c][2] (V - 128) + 2^19) >> 20, 0, 255)   (arithmetic shift)
 * csc_host [10] (HOST pointer) = y0, then m row-major (rows R, G, B; columns Y, U, V), 20-bit fixed point; 0 <= y0 <= 255 and
 * 255 * (|m[c][0]| + |m[c][1]| + |m[c][2]|) + 2^19 < 2^31.  Chroma is replicated, never interpolated: NV12 reads
 * uv[(r >> 1) * pitch + 2 (x >> 1) + {0, 1}] (an odd crop_top therefore changes the chroma parity of the cropped rows), YUYV
 * Y = row[2 x], U, V = row[4 (x >> 1) + {1, 3}].  Flip mirrors x before the colour lookup.  From the 8-bit colours on everything
 * is phnet_preprocess_u8 bit for bit (same tables, taps, rounding, normalisation, layouts, out_u8).  Bytes of a row beyond W0
 * (2 W0) and rows beyond H0 are never read.  PHNET_ERR_ARG before any launch: odd W0, odd H0 with NV12, pitch or chroma_offset
 * too small, frame_stride smaller than the bytes a frame spans, unknown format / layout, crop_top outside [0, H0), a null
 * pointer, a zero std, a matrix outside the bound above.  T == 0 is a no-op. */
int phnet_preprocess_yuv(const uint8_t* frames, float* out, uint8_t* out_u8,
                         const int32_t* xi, const int16_t* xc, const int32_t* yi, const int16_t* yc,
                         int32_t T, int32_t H0, int32_t W0, int32_t crop_top, int32_t out_h, int32_t out_w, int32_t flip, int32_t layout,
                         int32_t format, int64_t frame_stride, int32_t pitch, int64_t chroma_offset,
                         const int32_t* csc_host, const float* mean3_host, const float* std3_host, void* stream);

/* ---- training augmentation of a clip (csrc/augment.hip): the point-wise ops and the affine of the reference's imgaug pipeline
 * (transforms.py:190-249: HorizontalFlip, ChannelShuffle, MultiplyAndAddToBrightness, AddToHueAndSaturation, Dropout / CoarseDropout,
 * Affine with mode = 'constant', cval = 0) on the RESIZED 8-bit image, in the reference's order with the affine last, in one launch and
 * without an intermediate image; its blurs and edge filters are rule 7, behind phnet_augment_stencil_u8 below.  PARITY UNPINNED against
 * imgaug / cv2 (DESIGN.md "Training augmentation"): the rules below are the definition.
 * frames u8 [T][H][W][3] on the device (the out_u8 of phnet_preprocess_u8 / _yuv); out f32 NCHW [T][3][H][W] (layout 0) or NHWC4
 * [T][H][W][4] (layout 1); out_u8 optional [T][H][W][3], the augmented 8-bit image; mean3 / std3 HOST pointers.  Per-frame parameters,
 * all on the device and read by the kernel (a replayed graph sees what they hold then): flip2 i32 [T]; inv f64 [T][6], the
 * output -> source matrix a, row-major 2 x 3; table i32 [T][16] with columns 0-2 perm, 3 mq, 4 add, 5 value, 6 dropout mode, 7
 * per_channel, 8 threshold (the uint32 bits), 9 gh, 10 gw, 11 / 12 the low / high 32 bits of the frame's seed, 13-15 unused.
 * Output pixel (x, y) of frame t, pixel centres at integer coordinates:
 *   1. u = (a00 x + a01 y) + a02, v = (a10 x + a11 y) + a12, in float64, not contracted.
 *   2. if not (-2 < u < W + 1 and -2 < v < H + 1) - no tap can be inside; NaN included - the pixel is the fill colour 0, 0, 0.  Else
 *      U = floor(u * 32 + 0.5), x0 = U >> 5, fx = U & 31, and y0, fy from v alike: four taps (x0 + i, y0 + j), i, j in {0, 1}, with the
 *      weights (32 - fx, fx) x (32 - fy, fy), which sum to 1024.
 *   3. a tap (xt, yt) outside [0, W) x [0, H) is 0, 0, 0.  An inside tap is the source pixel (flip2 ? W - 1 - xt : xt, yt) taken through
 *      rule 4 and then rule 5 at (xt, yt).
 *   4. colour, in integers, in this order; an op with neutral parameters is skipped, so it returns its input bytes:
 *      a. c'[k] = c[perm[k]] (entries clamped to 0..2; neutral 0, 1, 2).
 *      b. brightness, V = max(R, G, B): V' = clamp(((V * mq + 128) >> 8) + add, 0, 255), mq = rint(mul * 256) clamped to [0, 65536], add
 *         to [-255, 255] (neutral 256, 0).  V = 0: R = G = B = V'.  Else every channel c = (2 c V' + V) / (2 V).
 *      c. hue and saturation, `value` clamped to [-255, 255] (neutral 0; imgaug's AddToHueAndSaturation: a hue turn of value * 360 / 255
 *         degrees, value added to S on a 0..255 scale), in an HSV with 24576 hue steps per turn:  V = max, C = V - min,
 *         S = V ? (510 C + V) / (2 V) : 0;  h = 0 if C = 0, else with (base, d) = (0, G - B) if V = R, else (8192, B - R) if V = G, else
 *         (16384, R - G):  h = (base + ((d + C) * 8192 + C) / (2 C) - 4096) mod 24576.  S' = clamp(S + value, 0, 255),
 *         C' = (2 V S' + 255) / 510,  h' = (h + floor((value * 49152 + 255) / 510)) mod 24576,  i = h' >> 12, f = h' & 4095,
 *         p = V - C', q = V - ((C' f + 2048) >> 12), t = V - ((C' (4096 - f) + 2048) >> 12);  (R, G, B) = (V, t, p), (q, V, p),
 *         (p, V, t), (p, q, V), (t, p, V), (V, p, q) for i = 0 .. 5.  Divisions are of non-negative integers; mod is non-negative.
 *   5. dropout, mode = column 6: 0 (or anything but 1, 2) none.  1, per pixel: element e = (t H + yt) W + xt.  2, coarse: the cell
 *      (cy, cx) = ((yt gh) / H, (xt gw) / W) of a gh x gw grid (each clamped to [1, 32768]; nearest-neighbour up-sampling of the
 *      mask), e = (t gh + cy) gw + cx.  per_channel = 0: all three channels become 0 iff phnet_rng_keep(seed, e, threshold) is false;
 *      else channel k becomes 0 iff phnet_rng_keep(seed, 3 e + k, threshold) is false.  phnet_rng_keep(seed, idx, thr) =
 *      (mix64(seed + (idx + 1) * 0x9E3779B97F4A7C15) >> 32) >= thr with the splitmix64 finaliser mix64 (csrc/common.h), all mod 2^64:
 *      an element is dropped with probability thr / 2^32.
 *   6. per channel (sum over the taps of weight * tap + 512) >> 10; then q / 255 and (v - mean) / std in f32, layouts as in
 *      phnet_preprocess_u8.
 * With the identity matrix one tap has the weight 1024; with neutral colour and no dropout the outputs equal phnet_preprocess_u8's on
 * the same frames bit for bit.  PHNET_ERR_ARG before any launch: a null pointer (out_u8 excepted), an unknown layout, H or W outside
 * [1, 32768], H * W * 4 or T * ceil(H W / 256) not below 2^31, a zero std.  T == 0 is a no-op.  Values in the tables cannot be checked
 * by the entry: the kernel clamps them as stated, so no table makes it read or write out of bounds. */
int phnet_augment_u8(const uint8_t* frames, float* out, uint8_t* out_u8, const int32_t* flip2, const double* inv, const int32_t* table,
                     int32_t T, int32_t H, int32_t W, int32_t layout, const float* mean3_host, const float* std3_host, void* stream);

/* phnet_augment_u8 with the neighbourhood ops of the reference's 'complex' recipe (transforms.py:220-238: EdgeDetect / DirectedEdgeDetect
 * between the hue change and the dropout, MotionBlur / MedianBlur / GaussianBlur between the dropout and the affine), csrc/
 * augment_stencil.hip.  PARITY UNPINNED against imgaug / cv2 like rules 1-6: rule 7 is the definition; op order, borders and the meaning
 * of the parameters follow imgaug's and OpenCV's documentation - filter2D and GaussianBlur with BORDER_REFLECT_101, medianBlur with
 * BORDER_REPLICATE, OpenCV's defaults for the calls imgaug makes, written down from memory.
 * The arguments of phnet_augment_u8, and: stencil i32 [T][40] on the device, read by the kernels like the other tables, with columns
 * 0 edge filter on (non-zero), 1-9 the edge weights e row-major, 10 blur kind, 11 k, 12-36 the first k * k entries m row-major (kind 1)
 * or the first k entries g (kind 3), 37-39 zero; staged u8 [T][H][W][3], scratch on the device that the caller owns, neither `frames`
 * nor `out_u8`.
 *   7. All coordinates are those of the flipped source image, the (xt, yt) of rule 3.
 *      r(i, n), reflect-101: 0 if n = 1; else with p = 2 (n - 1) and i' = i mod p (non-negative): i' if i' < n, else p - i'.  Defined
 *      for every i, so an image may be smaller than a radius.
 *      C(x, y): rule 4 on the source pixel (flip2 ? W - 1 - x : x, y).
 *      E(x, y): C(x, y) with the edge filter off.  On, per channel: clamp((sum over dy, dx in {-1, 0, 1} of e[dy + 1][dx + 1] *
 *      C(r(x + dx, W), r(y + dy, H)) + 2048) >> 12, 0, 255), e signed Q12, each weight clamped to [-65536, 65536], >> arithmetic.
 *      D(x, y): rule 5 at (x, y) applied to E(x, y), with the element indices of rule 5.
 *      B(x, y), by the blur kind; k is clamped to [3, 5] (kinds 1, 2) or [3, 9] (kind 3) and an even k is raised by one, R = k / 2:
 *        0, and every kind but 1, 2, 3: D(x, y).
 *        1, a k x k convolution (motion blur): clamp((sum over j, i in [0, k) of m[j][i] * D(r(x + i - R, W), r(y + j - R, H)) + 2048)
 *           >> 12, 0, 255), m Q12, each weight clamped to [0, 65536].
 *        2, a k x k median: per channel the median of the k * k values D(clamp(x + i - R, 0, W - 1), clamp(y + j - R, 0, H - 1)).
 *        3, a separable Gaussian: clamp((sum over j of g[j] * (sum over i of g[i] * D(r(x + i - R, W), r(y + j - R, H))) + 32768) >> 16,
 *           0, 255), g Q8, each weight clamped to [0, 256]; nothing is rounded between the two passes.
 *      Rule 3 then reads: an inside tap (xt, yt) is B(xt, yt).  For a frame with the edge filter off and blur kind 0 that is rule 3 as it
 *      stands above, and the frame's bytes are phnet_augment_u8's.
 * Two launches: the staging launch writes B of every frame that has the edge filter on or a blur kind 1-3 into `staged` (workgroups of
 * the other frames return at once: the launch is the same whatever the table holds, so a captured graph stays valid), the image launch
 * reads the taps of those frames from `staged` and runs rules 4, 5 itself on the others.  stencil == NULL is phnet_augment_u8, one launch
 * and bit for bit; so is an all-zero stencil table.  PHNET_ERR_ARG as phnet_augment_u8, and: a null `staged` with a non-null stencil,
 * T * ceil(W / 64) * ceil(H / 16) not below 2^31.  The kernels clamp what they read from the table as stated: no table contents make
 * them read or write out of bounds. */
int phnet_augment_stencil_u8(const uint8_t* frames, float* out, uint8_t* out_u8, const int32_t* flip2, const double* inv,
                             const int32_t* table, const int32_t* stencil, uint8_t* staged, int32_t T, int32_t H, int32_t W, int32_t layout,
                             const float* mean3_host, const float* std3_host, void* stream);

/* ---- lane IoU of the CULane-style evaluator: replaces LaneCompare::get_lane_similarity's two
 * cv::Mat canvases + cv::line + cv::sum (evaluation/culane/src/lane_compare.cpp:11-57).  A lane is a bit mask
 * [height][ceil(width/32)] uint32 in device memory.  phnet_lane_raster ORs thick segments into masks the caller zeroed: segs
 * [n_segs][5] int32 = (x0, y0, x1, y1, lane) with end points inside +-8192 (the cvRound'ed points of the interpolated lane);
 * a pixel is set iff its centre lies within lane_width/2 of the segment (exact integer test; parity against OpenCV's scan
 * conversion of the same segment unpinned - see oracle/culane_cpu.py).  phnet_lane_mask_stats adds the set bits of every mask to
 * area[n_lanes] and of masks[pairs[p][0]] & masks[pairs[p][1]] to inter[n_pairs] (int64, zeroed by the caller).
 * height, width <= 4096; lane_width <= 256; n_lanes + n_pairs <= 65535. ---- */
int phnet_lane_raster(const int32_t* segs, int64_t n_segs, uint32_t* masks, int32_t n_lanes, int32_t height, int32_t width,
                      int32_t lane_width, void* stream);
int phnet_lane_mask_stats(const uint32_t* masks, int32_t n_lanes, int32_t height, int32_t width, const int32_t* pairs,
                          int32_t n_pairs, int64_t* area, int64_t* inter, void* stream);
/* IoU MATRICES straight from the masks of phnet_lane_raster (the temporal evaluator, evaluation/evalTemporalOLV2.py:26-35,
 * and any caller that wants matrices instead of counts).  groups [n_groups][5] int32 in device memory = (row_first, n_rows,
 * col_first, n_cols, out_first): group g is the matrix of lanes row_first.. against lanes col_first.., its entry (r, c) is
 * iou[out_first + r * n_cols + c]; out_first[0] = 0 and out_first[g + 1] = out_first[g] + n_rows * n_cols (n_rows or n_cols
 * may be 0); n_entries = their total, passed by the caller because the host never reads `groups`.  With I, A, B the set bits
 * of a & b, a, b (int64) and U = A + B - I:  iou = (double)(scale * I) / ((double)(scale * U) + eps) - integer products,
 * one conversion each, one double add, one IEEE divide (no floating multiply, so nothing to fuse).  scale = 1, eps = 0 is
 * I / (A + B - I) with 0 / 0 = NaN; scale = 3, eps = 1e-10 the reference's three-channel canvases.  area (may be NULL) [n_lanes]
 * int64 receives every lane's set bits.  One workgroup per entry (and per lane for `area`) reads both masks once; no atomics:
 * every iou[0 .. n_entries) and every area[lane] is written on every call, nothing has to be zeroed, the result does not
 * depend on scheduling.  An entry whose lane index is outside [0, n_lanes), or that the table does not cover, is skipped.
 * height, width 1..4096; scale >= 1; eps finite and >= 0; n_entries + n_lanes < 2^31; n_groups == 0 or n_entries == 0
 * without `area` is a no-op. */
int phnet_lane_iou_groups(const uint32_t* masks, int32_t n_lanes, int32_t height, int32_t width, const int32_t* groups,
                          int32_t n_groups, int64_t n_entries, int32_t scale, double eps, double* iou, int64_t* area,
                          void* stream);

/* ---- validation F1 on the device (csrc/lane_eval.hip; DESIGN.md "Validation F1"): the host arithmetic of the CULane-style
 * evaluator around the two kernels above - the text files of evaluation/generate_lane.py:46-61, the chord-length spline of
 * evaluation/culane/src/spline.cpp, the cv::line end points of lane_compare.cpp:22-49, the Kuhn-Munkres matching of
 * include/hungarianGraph.hpp:39-67 and the counters of counter.cpp:83-161 - as two launches without a host synchronisation.  The
 * pixel work between them is phnet_lane_raster and phnet_lane_iou_groups, unchanged.
 *
 * phnet_lane_eval_segments: one launch for F images, one workgroup per lane.  points f32 [F][L][S][2], count i32 [F][L],
 * lanes_num i32 [F] as phnet_lane_points writes them; gt_points f32 [F][G][P][2], gt_count i32 [F][G], gt_num i32 [F]: the
 * annotations in evaluator coordinates (what the evaluator reads from the annotation file).  Out, every element written on every
 * call: segs i32 [F*(G+L)][C][5] with C = (max(S, P) - 1) * 50, rows (x0, y0, x1, y1, lane); lane_pts i32 [F][G+L].  Annotation g
 * of image f is lane f*(G+L)+g, prediction k is lane f*(G+L)+G+k; a lane's rows start at lane*C and its unused rows carry lane -1,
 * which phnet_lane_raster skips.  lane_pts is -1 for a lane that is not in the evaluator's list, else its number of points.
 * All arithmetic in double, nothing contracted into an fma, unless a rule says otherwise:
 *   1. presence.  Annotation g is present iff g < clamp(gt_num, 0, G), with clamp(gt_count, 0, P) points.  Prediction k is present
 *      iff k < clamp(lanes_num, 0, L) and - in wire mode only - clamp(count, 0, S) > 2 (the len(pts) > 2 filter of the writer), with
 *      clamp(count, 0, S) points.
 *   2. mode 0, wire (the writer followed by the evaluator's reader): points are taken last to first, vx = (double(tx) * size_w) / 2,
 *      vy = (double(ty) * size_h + crop_top) / 2, then each goes through the one-decimal text round trip: q = v * 10, k = rint(q); if
 *      q is exactly a half-integer and the exact residual fma(v, 10, -q) is not zero, k is the neighbour on the side of the
 *      residual; the value is float32(k / 10.0).  NaN and +-inf pass through.  mode 1, raw: the points are evaluator coordinates
 *      in evaluator order already and are used as they are.
 *   3. spline.  n >= 3 points: spline_interp_times(lane, 50) operation for operation - d[i] = p[i+1] - p[i], h[i] =
 *      sqrt(dx*dx + dy*dy); A[i] = h[i], B[i] = 2*(h[i] + h[i+1]), C[i] = h[i+1], D[i] = 6*(d[i+1]/h[i+1] - d[i]/h[i]);  C[0] /= B[0],
 *      D[0] /= B[0]; for i = 1..n-3: tmp = B[i] - A[i]*C[i-1], C[i] /= tmp, D[i] = (D[i] - A[i]*D[i-1]) / tmp;  M[n-2] = D[n-3], for
 *      i = n-4..0: M[i+1] = D[i] - C[i]*M[i+2]; M[0] = M[n-1] = 0.  Interval i, k = 0..49: t = (h[i]/50)*k, b = d[i]/h[i] -
 *      ((2*h[i])*M[i] + h[i]*M[i+1])/6, c = M[i]/2, dd = (M[i+1] - M[i])/(6*h[i]); the point is a + b*t + c*(t*t) + dd*((t*t)*t) with
 *      a = p[i], cast to float32 (the product form is the rule: pow(t, 3) is not correctly rounded by contract); the last input
 *      point is appended.  n == 2: the two points as they are.  n < 2: no segments.
 *   4. end points: the float32 value as a double, NaN -> 0, rint (ties to even), clamp to +-8192; consecutive points form the rows.
 * No table content causes an access outside the tables: every count read from memory is clamped before use.
 * Limits (PHNET_ERR_ARG before any launch): 1 <= G, L <= PHNET_LANE_EVAL_MAX_LANES, 2 <= S, P <= PHNET_LANE_EVAL_MAX_POINTS, 1 <= F,
 * F*(G+L)*C < 2^31, mode 0 or 1, size_h, size_w, crop_top finite, all pointers non-null.
 *
 * phnet_lane_eval_count: one launch, one workgroup walks the F images.  iou f64 [F][G][L] is phnet_lane_iou_groups (scale = 1,
 * eps = 0) on the static table (f*(G+L), G, f*(G+L)+G, L, f*G*L); lane_pts as above; video i32 [F] (may be NULL = row 0): the
 * accumulator row of each image, an image whose row is outside [0, V) is in no total.  Per image, count_im_pair on make_match
 * exactly as written:
 *   - the present annotations and predictions are compacted in order (n_anno rows, n_detect columns);
 *   - sim[r][c] = 0 where either lane has fewer than 2 points, else the iou entry; a NaN stays a NaN;
 *   - both sides empty: iou_im = 1; no annotation: fp = n_detect; no prediction: fn = n_anno;
 *   - else Kuhn-Munkres on sim, transposed when n_anno > n_detect: row weights start at -1e5 and rise by `w < m ? m : w`, column
 *     weights at 0; an edge is tight iff |lw + rw - m| < 1e-2; the search of a row visits columns in ascending order and re-enters
 *     through the row a taken column is matched to; after a failed search dmin = 1e10 and then `d < dmin ? d : dmin` over the
 *     (visited row, unvisited column) pairs; dmin == 1e10 ends the whole matching, else visited rows lose dmin, visited columns
 *     gain it and the search repeats;
 *   - a matched annotation adds its sim to the sum and is a true positive iff sim > threshold, else its match is withdrawn;
 *     tp, fp = n_detect - tp, fn = n_anno - tp, iou_im = sum / n_detect.
 * The relabelling passes of one image are capped at PHNET_LANE_EVAL_RELABEL_CAP: a failed search adds at least one column to the
 * visited set of the next, so a row needs at most 16 passes and an image at most 16 * 16 = 256 on any matrix without infinities;
 * the cap is four times that.  An image that reaches it counts as unmatched (tp = 0, fp = n_detect, fn = n_anno, iou_im = 0, no
 * match) and adds 1 to overflow[0]: the kernel cannot spin.
 * Out, per image, every element written on every call: tp, fp, fn i32 [F], iou_im f64 [F], anno_match i32 [F][G] (the caller's
 * prediction index k of annotation g, -1 = none).  Totals, zeroed by the caller at reset and ADDED to: totals i64 [V][4] = (tp, fp,
 * fn, images), iou_tot f64 [V], overflow i32 [1].  After a workgroup barrier one thread adds the images in ascending order, so the
 * double sum has the host's order and does not depend on scheduling; no float atomics.
 * Limits (PHNET_ERR_ARG before any launch): 1 <= G, L <= PHNET_LANE_EVAL_MAX_LANES, 1 <= F < 2^22, V >= 1, all pointers but `video`
 * non-null. */
#define PHNET_LANE_EVAL_MAX_LANES 16
#define PHNET_LANE_EVAL_MAX_POINTS 256
#define PHNET_LANE_EVAL_RELABEL_CAP 1024
int phnet_lane_eval_segments(const float* points, const int32_t* count, const int32_t* lanes_num, const float* gt_points,
                             const int32_t* gt_count, const int32_t* gt_num, int64_t F, int32_t G, int32_t L, int32_t S, int32_t P,
                             int32_t mode, double size_h, double size_w, double crop_top, int32_t* segs, int32_t* lane_pts,
                             void* stream);
int phnet_lane_eval_count(const double* iou, const int32_t* lane_pts, int64_t F, int32_t G, int32_t L, double threshold,
                          const int32_t* video, int32_t V, int32_t* tp, int32_t* fp, int32_t* fn, double* iou_im,
                          int32_t* anno_match, int64_t* totals, double* iou_tot, int32_t* overflow, void* stream);

/* ---- mask-level video metrics: the integer counts behind region similarity J and boundary F-measure F of a predicted and an
 * annotated mask per frame (csrc/mask_metrics.hip; replaces the host work of evaluation/evaluate_vid.py:51-57 with
 * video_metrics/jaccard.py and video_metrics/f_boundary.py: seg2bmap, two skimage binary_dilation(disk) calls and five np.sum per
 * frame pair).  pred, gt u8 [n_frames][height][width], packed - for instance the label maps of phnet_lane_draw.  One memset node and
 * two launches, no host synchronisation; integers only, so the counts do not depend on scheduling.
 *   1. foreground: a pixel is foreground iff its byte is not 0; label values 1..255 all count (np.where(img > 0, 1, 0),
 *      evaluate_vid.py:51-52).
 *   2. boundary map b (seg2bmap, f_boundary.py:107-118, the path without resampling): with s = seg[y][x], e = seg[y][x+1],
 *      so = seg[y+1][x], se = seg[y+1][x+1]:  y < H-1 and x < W-1: b = (s^e) | (s^so) | (s^se);  last row, x < W-1: b = s^e;  last
 *      column, y < H-1: b = s^so;  the bottom-right pixel: b = 0.  A mask that is all foreground has an empty boundary map.
 *   3. dilation: a pixel of dil(B) is set iff a set pixel of B lies at an offset (dx, dy) with dx^2 + dy^2 <= radius^2; nothing is
 *      set outside the image.  skimage's disk(radius) under binary_dilation.  The half-width of the disk's row dy is the integer
 *      square root of radius^2 - dy^2.  PARITY UNPINNED against skimage (not in the reference tree; the fixture pins scipy's
 *      binary_dilation with the same footprint).
 *   4. counts i64 [n_frames][7], in this order: area_pred, area_gt, area_both (foreground pixels of pred, gt, both), n_fg = |b_pred|,
 *      n_gt = |b_gt|, fg_match = |b_pred & dil(b_gt)|, gt_match = |b_gt & dil(b_pred)|.  Every element is written on every call,
 *      whatever `counts` and the workspace held.
 *   5. limits: 1 <= height, width <= PHNET_MASK_METRICS_MAX_SIZE (the renderer's), 0 <= radius <= PHNET_MASK_METRICS_MAX_RADIUS
 *      (0.008 x the diagonal of 4096 x 4096 is 47), n_frames >= 0; n_frames = 0 returns 0 and does nothing.  workspace: 8-byte aligned,
 *      at least phnet_mask_metrics_workspace(...) = n_frames * 2 * height * ceil(width / 64) * 8 bytes (the two boundary maps as
 *      64-pixel words; 0 for arguments outside the limits).  PHNET_ERR_ARG before any GPU call: a size, radius or n_frames outside the
 *      limits, a null pred / gt / counts / workspace, a misaligned or too small workspace (its size is a function of the other
 *      arguments, so it is one of them), n_frames * 2 * ceil(height / 32) * ceil(width / 512) >= 2^31. */
#define PHNET_MASK_METRICS_MAX_RADIUS 127
#define PHNET_MASK_METRICS_MAX_SIZE 4096
uint64_t phnet_mask_metrics_workspace(int32_t n_frames, int32_t height, int32_t width, int32_t radius);
int phnet_mask_metrics(const uint8_t* pred, const uint8_t* gt, int32_t n_frames, int32_t height, int32_t width, int32_t radius,
                       void* workspace, uint64_t workspace_bytes, int64_t* counts, void* stream);

/* ---- MaxPool2d(3,2,1): libs/models/resnet.py:217,297 ---- */
int phnet_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* argmax, int32_t N, int32_t Hi, int32_t Wi, int32_t C, void* stream);
int phnet_maxpool3x3s2_bwd(const float* dy, const uint8_t* argmax, float* dx, int32_t N, int32_t Hi, int32_t Wi, int32_t C, void* stream);

/* ---- FPN top-down add: laterals[i-1] += F.interpolate(laterals[i], size=..., mode='nearest') (libs/models/fpn.py:127-141) ---- */
int phnet_upsample_add(float* fine, const float* coarse, int32_t N, int32_t H, int32_t W, int32_t h, int32_t w, int32_t C, void* stream);
int phnet_upsample_add_bwd(const float* dfine, float* dcoarse, int32_t N, int32_t H, int32_t W, int32_t h, int32_t w, int32_t C, void* stream);

/* ---- LayerNorm (+residual)(+ReLU): replaces F.layer_norm at Router.py:72-81, utils/dynamic_head.py:42-58,
 * utils/transformer.py:275-298.  rows x L, affine w/b [L]; y = relu?(LN(x)*w + b (+res)). ---- */
int phnet_layernorm_fwd(const float* x, const float* w, const float* b, const float* res, float* y,
                        float* mean, float* rstd, int64_t rows, int32_t L, float eps, int32_t relu, void* stream);
uint64_t phnet_layernorm_bwd_workspace(int64_t rows, int32_t L);
int phnet_layernorm_bwd(const float* dy, const float* x, const float* y, const float* w,
                        const float* mean, const float* rstd, float* dx, float* dres, float* dw, float* db,
                        int64_t rows, int32_t L, int32_t relu, int32_t param_accumulate,
                        void* workspace, uint64_t ws_bytes, void* stream);

/* ---- routing-gate depth-wise 3x3: replaces Conv2d(N,N,3,padding=1,groups=N) (libs/models/Router.py:55-61).
 * x,y [N][C][P] planes (one per anchor), w [N][3][3], bias [N] or NULL; flip=1 computes the data gradient. ---- */
int phnet_dwconv3x3(const float* x, const float* w, const float* bias, float* y,
                    int32_t N, int32_t C, int32_t P, int32_t flip, void* stream);
int phnet_dwconv3x3_wgrad(const float* dy, const float* x, float* dw, float* db,
                          int32_t N, int32_t C, int32_t P, int32_t accumulate, void* stream);

/* ---- label assignment: replaces dynamic_assign.assign + scipy linear_sum_assignment on a .cpu() copy
 * (libs/utils/dynamic_assign.py:128-190) with one device launch.  pred [N][6+S], tgt [L][6+S] (col 1 == 1 = valid),
 * N <= 256, L <= 4.  rows_by_col [L] i64 (anchor matched to label j, -1 = none), rows_sorted [L] i64 (matched anchors
 * ascending, -1 padded), n_valid (optional) i32, cost (optional) [N][L] f32 (the solver's matrix, +inf = invalid).
 * PRECONDITION: N >= the number of valid label rows.  The flags are device data, so the host cannot reject a violation;
 * the kernels then report NO match at all (every row -1, n_valid 0, no pairs; the cost is still written) and the criteria
 * below reduce to their classification terms - the same holds for every entry point that assigns (the three here,
 * phnet_clip_loss / phnet_frame_loss, phnet_frame_loss_variant).  A one-to-many round that finds fewer unretired anchors than
 * valid label rows ends the rounds the same way, keeping the pairs of the rounds before it. ---- */
int phnet_lane_assign(const float* pred, const float* tgt, int32_t N, int32_t L, int32_t S,
                      float img_w, float img_h, int64_t* rows_by_col, int64_t* rows_sorted,
                      int32_t* n_valid, float* cost, void* stream);
/* One-to-many assignment: libs/utils/dynamic_assign.py:292-357 `assignOne2Many` (focal-cost alpha 0.5; label j wants
 * k_j = max(1, int(sum of its 4 largest line IoUs)) anchors; rounds of the exact matching, each keeps the pairs at the
 * positions whose k is still positive and retires their anchors) in one launch.  rows / cols [16] i64 (anchor, label row),
 * the reference's pair order, -1 padded; n_pairs (optional) i32. */
int phnet_lane_assign_one2many(const float* pred, const float* tgt, int32_t N, int32_t L, int32_t S,
                               float img_w, float img_h, int64_t* rows, int64_t* cols, int32_t* n_pairs, void* stream);
/* phnet_lane_assign + phnet_memory_tokens on its result in one launch (the pair the training schedule issues after every branch-B
 * pass): feat [N][E] this frame's tokens, tokens [L+1][E] / valid u8 [L+1] the memory entry they leave (Router4OL.py:563-584). */
int phnet_lane_assign_tokens(const float* pred, const float* tgt, int32_t N, int32_t L, int32_t S, float img_w, float img_h,
                             int64_t* rows_by_col, int64_t* rows_sorted, const float* feat, int32_t E,
                             float* tokens, uint8_t* valid, void* stream);

/* ---- fused per-frame criterion: replaces Criterion4OL.loss4OneStep (libs/utils/loss4OLV3.py:34-82,100-123: assignment,
 * focal, smooth-L1, LaneIoU, gate-weighted combination) AND its autograd backward with two launches.
 * pred / gate / dpred are HOST arrays of device pointers: pred[6] = branch A stages 0..2 then branch B stages 0..2,
 * each [N][6+S]; gate[3] each [N]; dpred[6] each [N][6+S].  tgt [L][6+S], L <= 4, N <= 256.
 * Outputs: loss [1]; dpred, dgate [3][N] = d loss / d input for unit upstream gradient; rows_by_col / rows_sorted
 * [6][L] int64 matched anchors (-1 padded).  Scratch: focal [6][N], scalars [12]. ---- */
int phnet_frame_loss(const float* const* pred, const float* const* gate, const float* tgt,
                     int32_t N, int32_t L, int32_t S, float img_w, float img_h,
                     float cls_w, float reg_w, float iou_w,
                     float liou_half_width, float liou_img_h, float liou_img_w,
                     float* loss, float* const* dpred, float* dgate,
                     int64_t* rows_by_col, int64_t* rows_sorted, float* focal, float* scalars, void* stream);
/* The T frames of a clip in the SAME two launches (the criterion is called frame by frame, trainOLV3.py:150-171, and nothing
 * flows from one frame's loss to the next): pred [T*6] / gate [T*3] / dpred [T*6] host arrays of device pointers, frame-major;
 * tgt [T][L][6+S]; loss [T]; dgate [T][3][N]; rows_by_col / rows_sorted [T][6][L]; scratch focal [T][6][N], scalars [T][12].
 * T <= 8.  phnet_frame_loss is the T = 1 case. */
int phnet_clip_loss(const float* const* pred, const float* const* gate, const float* tgt, int32_t T,
                    int32_t N, int32_t L, int32_t S, float img_w, float img_h,
                    float cls_w, float reg_w, float iou_w,
                    float liou_half_width, float liou_img_h, float liou_img_w,
                    float* loss, float* const* dpred, float* dgate,
                    int64_t* rows_by_col, int64_t* rows_sorted, float* focal, float* scalars, void* stream);
/* the reference's other two criteria, fused the same way (csrc/loss_variants.hip; two launches per frame):
 * variant 1 = libs/utils/loss4OL.py:88-232 (per-pair terms summed by position, placed on the last stage's anchors),
 * variant 2 = libs/utils/loss4OLV2.py:12-186 (one-to-many assignment, up to 16 pairs per branch and stage).
 * pair_rows / pair_cols [6][16] int64 (-1 padded), rows_sorted [6][L] int64 (variant 1), scratch 6*N + 192 floats. */
int phnet_frame_loss_variant(int32_t variant, const float* const* pred, const float* const* gate, const float* tgt,
                             int32_t N, int32_t L, int32_t S, float img_w, float img_h,
                             float cls_w, float reg_w, float iou_w,
                             float* loss, float* const* dpred, float* dgate,
                             int64_t* pair_rows, int64_t* pair_cols, int64_t* rows_sorted, float* scratch, void* stream);

/* ---- lane prior update: replaces the tanh/tan/repeat/cat chain of forward_first/second (Router4OL.py:328-345) and its
 * backward.  priors [N][6+S]; head [N][HW] = (cls 2 | reg 4 | offsets S | zero pad); ys [S] = prior_ys. ---- */
int phnet_lane_update_fwd(const float* priors, const float* head, const float* ys, float* preds, float* lines,
                          int32_t N, int32_t S, int32_t HW, float img_w, float img_h, void* stream);
int phnet_lane_update_bwd(const float* dpreds, const float* dlines, const float* lines, const float* head,
                          const float* ys, float* dhead, float* dpriors,
                          int32_t N, int32_t S, int32_t HW, float img_w, float img_h, void* stream);

/* ---- ReLU backward through the saved output (fused-ReLU epilogues of the linears) ---- */
int phnet_relu_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream);

/* ---- fused depth-wise stack of the routing gate: pre_norm + 4 x relu(LN(dw(relu(LN(dw(x))))) + x)
 * (libs/models/Router.py:72-75) in one launch forward, one backward (+ one reduce).  x/out [N][C][P], C*P <= 3072.
 * params / grads: HOST arrays of 34 device pointers: pre_norm.weight, pre_norm.bias, then per block b = 0..3:
 * conv1.weight [N][9], conv1.bias [N], ln1.weight [C*P], ln1.bias, conv2.weight, conv2.bias, ln2.weight, ln2.bias.
 * saved: phnet_gate_stack_saved_floats() floats written by fwd (NULL = inference), read by bwd.
 * N planes may cover several frames: plane n belongs to anchor n % anchors (the per-anchor filters are [anchors][9], N % anchors
 * == 0); the filter gradients of such a batch go through per-plane partials and one more small reduce launch. ---- */
uint64_t phnet_gate_stack_saved_floats(int32_t N, int32_t C, int32_t P);
uint64_t phnet_gate_stack_bwd_workspace(int32_t N, int32_t C, int32_t P);
int phnet_gate_stack_fwd(const float* x, const float* const* params, float* out, float* saved,
                         int32_t N, int32_t anchors, int32_t C, int32_t P, float eps, void* stream);
int phnet_gate_stack_bwd(const float* gout, const float* x, const float* out, const float* const* params,
                         const float* saved, float* const* grads, int32_t N, int32_t anchors, int32_t C, int32_t P, float eps,
                         int32_t accumulate, void* workspace, uint64_t ws_bytes, void* stream);
/* the wave-per-plane forms of the two calls above (csrc/gate_wave.hip; C = 64, P = 36: what the model runs) - phnet_gate_stack_fwd /
 * _bwd dispatch to them where phnet_gate_wave_applies; `saved` then holds only the four block inputs [4][N][C*P] */
int phnet_gate_wave_applies(int32_t C, int32_t P);
int phnet_gate_wave_partial_planes(int32_t N);
int phnet_gate_wave_fwd(const float* x, const float* const* params, float* out, float* saved,
                        int32_t N, int32_t anchors, float eps, void* stream);
int phnet_gate_wave_bwd(const float* gout, const float* x, const float* out, const float* const* params, const float* saved,
                        float* const* grads, int32_t N, int32_t anchors, float eps, int32_t accumulate,
                        void* workspace, void* stream);

/* ---- fused attention core (heads of width 16, Lq/Lk <= 256): replaces the scale/bmm/mask/softmax/dropout/bmm chain inside
 * nn.MultiheadAttention (libs/models/utils/transformer.py:275-298) and its backward.  q/k/v/o and the gradients are
 * addressed with row strides (floats, multiples of 4, 16-byte aligned bases), heads packed along the row.  key_valid u8[Lk] optional; keep u8[H][Lq][Lk]
 * optional explicit dropout keep-mask (kept weights scaled by keep_scale); with keep == NULL, rng_state != NULL and
 * drop_p > 0 the mask is drawn in the kernel instead: element (h, q, k) of dropout site rng_call is kept iff a splitmix64
 * hash of (*rng_state, rng_call, element index) clears drop_p * 2^32, scale 1/(1-drop_p); the backward recomputes the
 * same bits (F.dropout inside nn.MultiheadAttention).  *rng_state is a device counter the caller bumps once per step.
 * lse [H][Lq].  B clips per launch: clip b owns rows [b*Lq, (b+1)*Lq) of q/o/dq and [b*Lk, (b+1)*Lk) of k/v/dk/dv; key_valid
 * [B][Lk], keep [B][H][Lq][Lk], lse [B][H][Lq]. ---- */
int phnet_attention_fwd(const float* q, const float* k, const float* v, const uint8_t* key_valid, const uint8_t* keep,
                        float* o, float* lse, int32_t B, int32_t Lq, int32_t Lk, int32_t H, int32_t E,
                        int64_t sq, int64_t sk, int64_t sv, int64_t so, float keep_scale,
                        const uint64_t* rng_state, uint64_t rng_call, float drop_p, void* stream);
int phnet_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* dout,
                        const float* lse, const uint8_t* key_valid, const uint8_t* keep,
                        float* dq, float* dk, float* dv, int32_t B, int32_t Lq, int32_t Lk, int32_t H, int32_t E,
                        int64_t sq, int64_t sk, int64_t sv, int64_t so, int64_t sdq, int64_t sdk, int64_t sdv,
                        float keep_scale, const uint64_t* rng_state, uint64_t rng_call, float drop_p, void* stream);

/* ---- transformer glue: `tgt + dropout(x)` and `dropout(gelu(x))` (libs/models/utils/transformer.py:275-298) as one launch
 * each, dropout bits from the same counter-based generator as the attention kernels (site id rng_call; drop_p = 0 or
 * rng_state = NULL: no dropout).  phnet_dropout_add with res = NULL is plain dropout, which is also its own backward. ---- */
int phnet_dropout_add(const float* x, const float* res, float* y, int64_t n,
                      const uint64_t* rng_state, uint64_t rng_call, float drop_p, void* stream);
int phnet_gelu_dropout_fwd(const float* x, float* y, int64_t n, const uint64_t* rng_state, uint64_t rng_call, float drop_p,
                           void* stream);
int phnet_gelu_dropout_bwd(const float* dy, const float* x, float* dx, int64_t n, const uint64_t* rng_state,
                           uint64_t rng_call, float drop_p, void* stream);

/* ---- small fused pieces of the per-frame loop ----
 * memory tokens (Router4OL.py:563-584, _tokens): rows i64[L] = positive anchors ascending, -1 padded; tokens [L+1][E] = their
 *   features, then the mean of all other anchors; valid u8[L+1].
 * gate tail (Router.py:76-80): gate = sigmoid(relu(h . w + b)) and its backward from the saved output.
 * stage hand-over (Router4OL.py:298-302): blended priors and their sampled x positions. ---- */
int phnet_memory_tokens(const float* feat, const int64_t* rows, float* tokens, uint8_t* valid,
                        int32_t B, int32_t N, int32_t E, int32_t L, void* stream);      /* B clips: leading dimension of all four */
int phnet_gate_tail_fwd(const float* h, const float* w, const float* b, float* out, int32_t N, int32_t K, void* stream);
int phnet_gate_tail_bwd(const float* dout, const float* out, const float* h, const float* w, float* dh, float* dw, float* db,
                        int32_t N, int32_t K, int32_t accumulate, void* stream);
int phnet_blend_priors(const float* gate, const float* a, const float* b, const int64_t* idx, float* priors, float* on_map,
                       int32_t N, int32_t W, int32_t P, void* stream);

/* ---- streaming inference: the cross-frame memory of B live video streams as a device-resident token ring (csrc/stream.hip;
 * replaces the host-side FIFO of Router4OL.py:555-556 and its per-frame torch.cat, so that ONE captured hipGraph serves every
 * frame of a video).  State, caller-allocated: ring [S][B][W][L+1][E], ring_valid u8 [S][B][W][L+1] (S stages, B streams,
 * W = save_freq_max slots, L = max_lanes);  n i32[B] = frames pushed since the stream's last reset (reset = the caller writes
 * n[b] = 0, stream-ordered; the ring need not be cleared);  cursor i32[B] = scratch word that carries n from window to push.
 * Per frame: window, (the frame's forward), push - no launch reads the word it advances.
 * phnet_stream_window: the memory the frame attends to, oldest remembered frame first, empty slots LAST (zero rows, marked
 *   invalid): window [S][B][W*(L+1)][E], window_valid u8 [S][B][W*(L+1)], has_memory u8[B] = n[b] > 0.  With c = min(n, W),
 *   logical slot j < c is physical slot (n - c + j) % W.  Also publishes cursor[b] = n[b].  E % 4 == 0.
 * phnet_stream_push: the memory entry of this frame for every stage and stream - phnet_memory_tokens of feat [S][B][N][E] and
 *   anchors_sorted i64[B][L] (-1 padded), bit-identical to it - written to physical slot cursor[b] % W; then n[b] = cursor[b] + 1.
 *   1 <= L < N, E <= 1024.
 * phnet_stream_select: feat[b] = attn[b] (both [B][N][E]) where has_memory[b] == 0, in place: the cross-frame decoder always
 *   runs in a captured step, and the streams without a memory take its input instead (Router4OL.py:349-353).  E % 4 == 0. ---- */
int phnet_stream_window(const float* ring, const uint8_t* ring_valid, const int32_t* n, int32_t* cursor, float* window,
                        uint8_t* window_valid, uint8_t* has_memory, int32_t S, int32_t B, int32_t W, int32_t E, int32_t L,
                        void* stream);
int phnet_stream_push(const float* feat, const int64_t* anchors_sorted, float* ring, uint8_t* ring_valid, const int32_t* cursor,
                      int32_t* n, int32_t S, int32_t B, int32_t W, int32_t N, int32_t E, int32_t L, void* stream);
int phnet_stream_select(const float* attn, const uint8_t* has_memory, float* feat, int32_t B, int32_t N, int32_t E, void* stream);

/* ---- streaming inference of the Router4OLV2 family (csrc/stream_v2.hip): the key set of the cross-frame decoder of ONE
 * refinement stage for B streams, one launch.  V2 runs the decoder on every frame: on the stream's memory window from frame
 * min_frames (= cfg.save_freq) after its reset on, on the frame's OWN tokens before (Router4OLV2.py:320-325).  The decision is
 * cursor[b] >= min_frames (and cursor[b] > 0: an empty memory is never a key set), cursor as phnet_stream_window published it.
 * local, tgt [B][N][E]; pos [N][E]; window [B][M][E] and window_valid u8 [B][M] = one stage of phnet_stream_window's output;
 * tgt = local + pos (written where phnet_stream_push reads it); keys [B][Kmax][E], keys_valid u8 [B][Kmax], Kmax >= max(N, M):
 * rows 0..M-1 = the window with its validity, or rows 0..N-1 = tgt, all valid; the rest zero / invalid.  E % 4 == 0. ---- */
int phnet_stream_keys(const float* local, const float* pos, const float* window, const uint8_t* window_valid,
                      const int32_t* cursor, float* tgt, float* keys, uint8_t* keys_valid, int32_t B, int32_t N, int32_t M,
                      int32_t Kmax, int32_t E, int32_t min_frames, void* stream);

/* ---- Router4OLV2 model family (what testOLV3.py imports; inference only - its training path cannot run as shipped) ----
 * phnet_gate_v2_fwd: AdaptiveRouter4LaneV2.forward (libs/models/Router.py:83-132) in one launch: Conv1d(k3, pad 1, no bias)
 *   + BatchNorm1d + ReLU, Conv1d(k1) + BatchNorm1d + ReLU, Flatten, Linear(C2*P -> P), mean over the P outputs, sigmoid.
 *   x [M][C][P]; w1 [C1][C][3]; s1 / t1 [C1] BatchNorm folded to conv * s + t; w2 [C2][C1]; s2 / t2 [C2]; wl [P][C2*P];
 *   bl [P]; out [M].
 * phnet_dyn_bmm_ln_relu_fwd_any: the two per-anchor products of DynamicConvV2 (libs/models/utils/dynamic_head.py:94-104) at
 *   run-time shapes (per-level widths 64/32/16, 24/48/96 sample points), forward only: y[n] = relu(LayerNorm_J(x[n] @ w[n])).
 * phnet_route_lines: RouterOL.forward, eval (libs/models/Router4OLV2.py:508-511): d = mean over the S stage gates, then
 *   hard != 0: out = d >= 0.5 ? b : a (torch.where);  hard == 0: out = b * d + a * (1 - d) (Router4OL.py:538-541).
 *   gates [S][M]; a (branch A), b (branch B), out [M][W].
 * The per-level ROI pooling is phnet_roi_pool_fwd with C < 64, the 8 x 32 attention phnet_attention_fwd with E = 32 H. */
int phnet_gate_v2_fwd(const float* x, const float* w1, const float* s1, const float* t1, const float* w2,
                      const float* s2, const float* t2, const float* wl, const float* bl, float* out,
                      int32_t M, int32_t C, int32_t P, int32_t C1, int32_t C2, void* stream);
int phnet_dyn_bmm_ln_relu_fwd_any(const float* x, const float* w, const float* gamma, const float* beta, float* y,
                                  int32_t N, int32_t P, int32_t K, int32_t J, float eps, void* stream);
int phnet_route_lines(const float* gates, const float* a, const float* b, float* out,
                      int32_t S, int32_t M, int32_t W, int32_t hard, void* stream);

/* ---- row-local chain of a pre-norm transformer layer in one launch, forward only (libs/models/utils/transformer.py:275-298
 * between the attention cores): [v = in @ Wa^T + ba; t = resid + dropout(v)] | t = in;  h = LayerNorm(t; ln1);
 * [f = dropout(gelu(h @ W1^T + b1)); t += dropout(f @ W2^T + b2); h = LayerNorm(t; ln2)];  [y = h @ Wg^T + bg].
 * in / resid / t_out / h_out [R][E], y_out [R][NG]; E = 128 (FF 256) or 256 (FF 512); optional parts are NULL.  Dropout sites as
 * in phnet_dropout_add (same generator, same element indices as the unfused kernels: a recomputation through those sees the
 * masks drawn here). ---- */
int phnet_rowchain_fwd(const float* in, const float* resid, const float* Wa, const float* ba, const float* ln1w, const float* ln1b,
                       const float* W1, const float* b1, const float* W2, const float* b2, const float* ln2w, const float* ln2b,
                       const float* Wg, const float* bg, float* t_out, float* h_out, float* y_out,
                       int32_t R, int32_t E, int32_t FF, int32_t NG, float eps,
                       const uint64_t* rng_state, uint64_t call_a, uint64_t call_f, uint64_t call_3, float drop_p, void* stream);

/* ---- [chain A] -> cross-attention core -> [chain B] of a pre-norm decoder layer in one launch, forward only: the bits of
 * phnet_rowchain_fwd -> phnet_attention_fwd -> phnet_rowchain_fwd.  B items as contiguous row blocks: item b owns rows
 * [b*Lq, (b+1)*Lq) of in / resid / the outputs and keys [b*Lk, (b+1)*Lk) of k / v (row strides sk / sv, heads packed along the row) /
 * key_valid u8[B*Lk] (optional).  Chain A (Wa0 != NULL): in = the self-attention output, resid its residual,
 * t = resid + dropout(in @ Wa0^T + ba0) [site call_a0], q = LayerNorm(t; ln0w, ln0b, eps0) @ Wq^T + bq; without it in = q and
 * resid = t of an earlier launch.  Attention weights: dropout site call_c, probability attn_drop_p.  Chain B: out-projection
 * Wa / ba [site call_a], LayerNorm ln1, feed-forward W1 / b1 / W2 / b2 [sites call_f, call_3], LayerNorm ln2, optional next
 * projection Wg / bg [NG][E]; outputs as in phnet_rowchain_fwd.  Supported: E = 128 = 16 H, FF = 256, 1 <= Lk <= 64; anything
 * else returns PHNET_ERR_ARG and launches nothing (the caller keeps the three launches). ---- */
int phnet_rowchain_attn_fwd(const float* in, const float* resid, const float* Wa0, const float* ba0, const float* ln0w,
                            const float* ln0b, const float* Wq, const float* bq, float eps0,
                            const float* k, const float* v, int64_t sk, int64_t sv, const uint8_t* key_valid,
                            const float* Wa, const float* ba, const float* ln1w, const float* ln1b,
                            const float* W1, const float* b1, const float* W2, const float* b2, const float* ln2w, const float* ln2b,
                            const float* Wg, const float* bg, float* t_out, float* h_out, float* y_out,
                            int32_t B, int32_t Lq, int32_t Lk, int32_t H, int32_t E, int32_t FF, int32_t NG, float eps,
                            const uint64_t* rng_state, uint64_t call_a0, uint64_t call_c, uint64_t call_a, uint64_t call_f,
                            uint64_t call_3, float drop_p, float attn_drop_p, void* stream);

/* ---- tower weights of a lane-head branch (libs/models/Router4OL.py:68-99, 308-326: T towers of two Linear + ReLU layers and one
 * Linear head each) assembled for the 3-GEMM chain, and their gradients scattered back: one launch each instead of the ~12
 * torch.cat / block_diag launches per branch and clip and the ~40 of their autograd backward.  params / grads: HOST arrays of 6*T
 * device pointers (per tower: layer-1 weight [C][C], bias [C], layer-2 weight, bias, head weight [o_t][C], head bias [o_t]).
 * The assembled tensors live in ONE buffer w1 [TC][C] | b1 [TC] | w2 [TC][TC] | b2 [TC] | wh [HW][TC] | bh [HW]
 * (phnet_tower_layout: its size, the six offsets, HW = sum o_t rounded up to a multiple of 4). ---- */
uint64_t phnet_tower_layout(int32_t T, int32_t C, const int32_t* head_out, int64_t* offsets, int32_t* hw);
int phnet_assemble_towers(const float* const* params, int32_t T, int32_t C, const int32_t* head_out, float* dst, void* stream);
int phnet_scatter_tower_grads(const float* src, float* const* grads, int32_t T, int32_t C, const int32_t* head_out,
                              int32_t accumulate, void* stream);

/* ---- towers + heads + lane prior update of a branch in one launch, forward only (libs/models/Router4OL.py:308-345): per tower
 * relu(x W1^T + b1) -> relu(. W2^T + b2) -> head; the heads concatenated are (cls 2 | reg 4 | offsets S); then the prior update of
 * phnet_lane_update_fwd.  params: HOST array of 6*T device pointers, used where they are (no assembled copies).  C = 64 or 128. ---- */
int phnet_tower_chain_fwd(const float* x, const float* const* params, int32_t T, int32_t C, const int32_t* head_out,
                          const float* priors, const float* ys, float* preds, float* lines, int32_t R, int32_t S,
                          float img_w, float img_h, void* stream);

/* ---- optimizer: one AdamW step (torch.optim.AdamW semantics, libs/utils/optimizer.py:33-35) over flat parameter / gradient /
 * moment arrays; elements [0, n_decay) get decoupled weight decay.  n % 4 == 0.  step: device int64, 1-based, already
 * incremented by the caller for this step.  lr_dev (optional): DEVICE pointer to the learning rate; when non-NULL it
 * replaces `lr`, so that a hipGraph-captured step follows an LR schedule (the host rewrites the scalar between replays). ---- */
int phnet_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_decay, const int64_t* step,
                     float lr, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* ---- guarded step: global-norm clip (torch.nn.utils.clip_grad_norm_, trainOL.py:221) and the non-finite skip of GradScaler.step
 * (trainOL.py:225-227) for the flat arenas, decided on the device: phnet_grad_guard, then phnet_adamw_step_guarded.  No host
 * synchronisation, no floating-point atomics, nothing to zero between steps; capturable.  The rules:
 *  1. S = sum of g_i^2 over all n elements (padding included), each square and every addition in float64, in an order fixed by n and
 *     PHNET_GUARD_CHUNK alone: element -> lane -> wavefront -> chunk partial -> ascending chunk index.  Chunk c holds elements
 *     [c CHUNK, min(n, (c+1) CHUNK)); its 4-element vector q belongs to lane q % 256; a lane adds the squares of component e of its
 *     vectors, in ascending q, into accumulator a_e, then takes (a0 + a1) + (a2 + a3); the 64 lanes of a wavefront (lanes 64w ..
 *     64w+63) are added by an xor butterfly over the lane distances 32, 16, 8, 4, 2, 1; the chunk partial is ((w0 + w1) + w2) + w3;
 *     S adds the chunk partials one by one in ascending c, starting from 0.  Two calls on the same buffer give the same bits,
 *     whatever the grid, the CU count or the arrival order of workgroups.
 *  2. nonfinite = the number of elements whose exponent field is all ones (an integer test on the bit pattern).
 *  3. inv = 1 / grad_scale[0] in f32 when grad_scale != NULL, else 1.  norm = fl32(sqrt(S) * (double)inv): the norm of the unscaled,
 *     unclipped gradient, what clip_grad_norm_ returns.
 *  4. coef = min(1, max_norm / (norm + 1e-6f)) in f32 with PHNET_GUARD_CLIP (torch's clip_coef, clamped), else 1.  A NaN norm gives a
 *     NaN coef, as in torch with error_if_nonfinite=False.
 *  5. mult = fl32(coef * inv); the update sees g_eff_i = fl32(g_i * mult), one rounded f32 multiply.  g itself is never written
 *     (torch's clip rewrites .grad in place; here .grad keeps the raw gradient).
 *  6. skip = PHNET_GUARD_SKIP_NONFINITE && (nonfinite > 0 || (found_inf != NULL && found_inf[0] != 0) || !isfinite(norm)).
 *  7. skip: p, m, v and step keep their bits; stats word 3 (skipped steps) += 1.
 *  8. otherwise: step[0] += 1, then phnet_adamw_step's element update on g_eff (one shared device function).
 * workspace: PHNET_GUARD_WS_BYTES_PER_CHUNK * ceil(n / PHNET_GUARD_CHUNK) bytes, 8-byte aligned (float64 partials, then uint32
 * counts; written before it is read, never zeroed).  stats: PHNET_GUARD_STATS_WORDS int64 words - 0: {f32 norm, f32 mult},
 * 1: this step was skipped (0 | 1), 2: nonfinite, 3: skipped steps in total (zero it once) - words 0-2 are written by every call.
 * grad_scale / found_inf: what torch.amp.GradScaler hands an optimizer with _step_supports_amp_scaling (one f32 each), or NULL.
 * n % 4 == 0; max_norm >= 0 (used only with PHNET_GUARD_CLIP; pass 0 without).
 * phnet_adamw_step_guarded: phnet_adamw_step with `mult` (stats word 0, second float) and `skip` (stats word 1) read on the
 * device; `step` is the counter phnet_grad_guard has already advanced. ---- */
#define PHNET_GUARD_CHUNK 131072
#define PHNET_GUARD_WS_BYTES_PER_CHUNK 12
#define PHNET_GUARD_STATS_WORDS 4
#define PHNET_GUARD_SKIP_NONFINITE 1
#define PHNET_GUARD_CLIP 2
int phnet_grad_guard(const float* g, int64_t n, void* workspace, uint64_t ws_bytes, int64_t* stats, int64_t* step,
                     float max_norm, int32_t flags, const float* grad_scale, const float* found_inf, void* stream);
int phnet_adamw_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_decay, const int64_t* step,
                             float lr, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                             const float* mult, const int64_t* skip, void* stream);

/* residual + dropout + LayerNorm of the pre-norm decoder layers in one launch: t = res + dropout(x), h = LN_L(t)*w + b
 * (L <= 256), and its backward (dt = gradient arriving on the residual stream, may be NULL): dres, dx, dw, db. */
int phnet_dropout_add_ln_fwd(const float* x, const float* res, const float* w, const float* b, float* t, float* h,
                             float* mean, float* rstd, int64_t rows, int32_t L, float eps,
                             const uint64_t* rng_state, uint64_t rng_call, float drop_p, void* stream);
int phnet_dropout_add_ln_bwd(const float* dh, const float* dt, const float* t, const float* w, const float* mean,
                             const float* rstd, float* dres, float* dx, float* dw, float* db,
                             int64_t rows, int32_t L, int32_t param_accumulate,
                             const uint64_t* rng_state, uint64_t rng_call, float drop_p,
                             void* workspace, uint64_t ws_bytes, void* stream);

/* ---- per-anchor dynamic convolution: y[n] = relu(LayerNorm_J(x[n] @ w[n]) * gamma + beta), replacing torch.bmm + norm1/norm2
 * + ReLU in libs/models/utils/dynamic_head.py:40-51 (and their backward).  x [N][P][K], w [N][K][J] (generated per anchor),
 * y [N][P][J], stats [N][P][2] = (mean, rstd) (NULL = inference).  J <= 128; J and K divide 256.  Backward: dx optional,
 * dw [N][K][J], dgamma/dbeta [J] overwritten or accumulated; workspace N*2*J floats. ---- */
int phnet_dyn_bmm_ln_relu_fwd(const float* x, const float* w, const float* gamma, const float* beta, float* y,
                              float* stats, int32_t N, int32_t P, int32_t K, int32_t J, float eps, void* stream);
int phnet_dyn_bmm_ln_relu_bwd(const float* dy, const float* x, const float* w, const float* y, const float* stats,
                              const float* gamma, float* dx, float* dw, float* dgamma, float* dbeta,
                              int32_t N, int32_t P, int32_t K, int32_t J, float eps, int32_t param_accumulate,
                              void* workspace, uint64_t ws_bytes, void* stream);
/* the matrix-pipe forms (csrc/dyn_mfma.hip: one wavefront per anchor, v_mfma_f32_16x16x4_f32, no LDS); the two calls above
 * dispatch to them where phnet_dyn_mfma_applies (P <= 36, (K, J) = (64, 128) or (128, 64)) */
int phnet_dyn_mfma_applies(int32_t P, int32_t K, int32_t J);
int phnet_dyn_mfma_fwd(const float* x, const float* w, const float* gamma, const float* beta, float* y, float* stats,
                       int32_t N, int32_t P, int32_t K, int32_t J, float eps, void* stream);
int phnet_dyn_mfma_bwd(const float* dy, const float* x, const float* w, const float* y, const float* stats, const float* gamma,
                       float* dx, float* dw, float* lnpart, int32_t N, int32_t P, int32_t K, int32_t J, void* stream);

/* ---- bias gradients: column sums of [M][C] ---- */
uint64_t phnet_colsum_workspace(int64_t M, int32_t C);
int phnet_colsum(const float* a, float* out, int64_t M, int32_t C, int32_t accumulate, void* workspace, uint64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
