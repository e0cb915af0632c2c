/*
 * rvhip.h — C ABI of the MI355X-native (gfx950) road-vision hot path.
 *
 * One shared library (librvhip.so, built by road-vision-system_amd/csrc/Makefile)
 * exports every function declared here.  Conventions, identical for every entry:
 *
 *   - plain pointers and sizes only; no torch / STL types cross the boundary;
 *   - device buffers are owned by the caller (torch tensors on the host side),
 *     the library never allocates or frees device memory inside a launch
 *     function, so every launch function is hipGraph-capturable;
 *   - `stream` is a hipStream_t passed as void* (NULL = legacy default stream);
 *     all work is stream-ordered, nothing synchronises the host;
 *   - return value: 0 = ok, RV_EINVAL (-1000) = bad argument (shape / pointer /
 *     capacity), RV_ECAP (-1001) = a capacity limit was exceeded, and
 *     -(hipError_t) for a HIP launch error.  Nothing throws across the ABI.
 *     rv_last_error() returns a static, thread-local description of the last
 *     non-zero status.
 *
 * Frames are interleaved BGR uint8, H x W x 3, `pitch` bytes between rows and
 * H*pitch bytes between frames of a batch (B frames = B independent camera
 * streams, stream-major).  Each entry cites the reference interface it
 * replaces (paths relative to YJxyzxyz/road-vision-system).
 */
#ifndef RVHIP_H
#define RVHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RV_OK 0
#define RV_EINVAL (-1000)
#define RV_ECAP (-1001)
#define RV_EOF 1 /* rv_capture_*: the source has no more frames */

/* ABI version (bumped on any signature change) and last-error text. */
int rv_abi_version(void);
const char* rv_last_error(void);
/* Measurement plumbing (no reference counterpart): an empty kernel whose
 * dispatch marks a point in a rocprofv3 kernel trace (bench.py brackets its
 * timed region with tags 1 and 2). */
int rv_trace_marker(int tag, void* stream);
/* Diagnostics (no reference counterpart): on a fatal signal write the native
 * stack to stderr, then chain to the previously installed handler (e.g.
 * Python's faulthandler).  Idempotent. */
int rv_install_crash_handler(void);

/* ------------------------------------------------------------------------ */
/* Preprocess: CLAHEDehaze (src/preprocess/ops/clahe_dehaze.py:13-32,       */
/* cv2.createCLAHE(...).apply on the Y plane of cv2.COLOR_BGR2YCrCb, then    */
/* cv2.COLOR_YCrCb2BGR) and MedianDerain (src/preprocess/ops/                */
/* median_derain.py:10-14, cv2.medianBlur).                                  */
/* ------------------------------------------------------------------------ */

/* Workspace bytes rv_clahe_ycrcb_u8 needs for B frames with a tiles x tiles
 * grid (one 256-entry u8 LUT per tile per frame). */
size_t rv_clahe_ws_bytes(int B, int tiles);

/* CLAHE on the luma of BGR frames, returned as BGR (YCrCb path of
 * clahe_dehaze.py:27-30).  `tiles` is the already-clamped grid
 * (clahe_dehaze.py:17: max(2, tile_grid)); `clip` the clipLimit.
 * in and out may not alias. */
int rv_clahe_ycrcb_u8(const uint8_t* in, uint8_t* out, int B, int H, int W,
                      int pitch, int tiles, double clip, void* ws,
                      size_t ws_bytes, void* stream);

/* CLAHEDehaze space="LAB" (clahe_dehaze.py:21-25): cv2.COLOR_BGR2LAB, CLAHE
 * on L, cv2.COLOR_LAB2BGR, 8U sRGB / D65 integer paths (OpenCV color_lab.cpp
 * RGB2Lab_b / Lab2RGBinteger, restated; csrc/lab.h).  Same arguments and
 * workspace as rv_clahe_ycrcb_u8.  The first LAB call on a device uploads
 * the Lab tables to it synchronously; call rv_lab_init() (current device)
 * once before capturing the op in a graph. */
int rv_clahe_lab_u8(const uint8_t* in, uint8_t* out, int B, int H, int W,
                    int pitch, int tiles, double clip, void* ws,
                    size_t ws_bytes, void* stream);
int rv_lab_init(void);
/* Host copy of the Lab tables (parity tests): {u16 gamma[256], cbrt[3072],
 * yf[512], invg[4096]; i32 cf[9], ci[9]}, exactly 15944 bytes. */
int rv_lab_tables_host(void* out, size_t bytes);

/* Exact per-channel k x k median with replicated borders (cv2.medianBlur on
 * 8UC3).  k is the already-normalised kernel size (median_derain.py:11-13:
 * odd, clamped to [3, 9]). in and out may not alias. */
int rv_median_u8c3(const uint8_t* in, uint8_t* out, int B, int H, int W,
                   int pitch, int k, void* stream);

/* The default chain [CLAHEDehaze(YCrCb), MedianDerain(k)] of
 * configs/default.yaml:21-31 in one pass over HBM after the LUT pass: CLAHE
 * apply + colour round trip + k x k median, writing `out` (the observable
 * `proc` frame of main_preview.py:94).  Bit-identical to calling
 * rv_clahe_ycrcb_u8 then rv_median_u8c3.  ws as for rv_clahe_ws_bytes. */
int rv_clahe_median_u8(const uint8_t* in, uint8_t* out, int B, int H, int W,
                       int pitch, int tiles, double clip, int k, void* ws,
                       size_t ws_bytes, void* stream);

/* 1 if rv_clahe_median_u8 can run this geometry (the LUT window of one
 * output tile fits in LDS), 0 if the caller must use the unfused pair. */
int rv_clahe_median_fits(int H, int W, int tiles, int k);

/* The default chain plus the detector's LetterBox in one pass:
 * rv_clahe_median_u8 (k = 3) writing `out`, and the Ultralytics letterbox of
 * `out` (geo from rv_letterbox_geometry) into lb_out (B x geo[0] x geo[1] x 3),
 * byte-identical to rv_clahe_median_u8 followed by rv_letterbox_u8.  Replaces
 * the pipeline -> detector hand-over of main_preview.py:99-101
 * (PreprocessPipeline.__call__ then YOLOUltralytics.infer's LetterBox,
 * src/detect/yolo_ultralytics.py:28-35).  RV_EINVAL unless
 * rv_clahe_median_letterbox_fits() says 1. */
int rv_clahe_median_letterbox_u8(const uint8_t* in, uint8_t* out, int B, int H, int W,
                                 int pitch, int tiles, double clip, int k, void* ws,
                                 size_t ws_bytes, uint8_t* lb_out, const int* geo,
                                 void* stream);

/* 1 if rv_clahe_median_letterbox_u8 supports this geometry: k = 3, the LUT
 * cells of a 128 x 32 tile fit in LDS and every letterbox pixel's bilinear
 * taps fall in one tile. */
int rv_clahe_median_letterbox_fits(int H, int W, int tiles, int k, const int* geo);

/* Low-contrast auto gate (src/preprocess/pipeline.py:24-30): per frame,
 * span_out[b] = max(gray) - min(gray), gray = cv2.COLOR_BGR2GRAY (14-bit
 * fixed point).  ws: 2*B ints of device scratch. */
int rv_gray_span_u8(const uint8_t* in, int B, int H, int W, int pitch,
                    int* ws, int* span_out, void* stream);

/* Dark-channel-prior dehaze (He, Sun, Tang), the inverse of the fog model
 * I = J t + A (1 - t) (no reference counterpart: the stronger dehaze the
 * reference's plugin registry leaves room for).  Integer arithmetic end to
 * end, every division a floor division, every window the square around the
 * pixel clipped to the frame (N pixels):
 *   d   = patch x patch minimum of min(B, G, R)
 *   n   = max(1, H W / 1000); L = the largest level with count(d >= L) >= n;
 *         M = {d >= L}, cnt = |M|; A_c = max(1, (2 sum_M I_c + cnt) / (2 cnt))
 *   nd  = patch x patch minimum of min_c min(255, (510 I_c + A_c) / (2 A_c))
 *   t0  = 255 - ((wq nd + 128) >> 8)
 *   radius 0: t = t0.  Otherwise a guided filter of t0 by the gray g of
 *   rv_gray_span_u8 over (2 radius + 1)^2: with the box sums N, Sg, Sp, Sgp,
 *   Sgg of 1, g, t0, g t0, g g:
 *         aq = ((N Sgp - Sg Sp) << 14) / (N Sgg - Sg^2 + eq N^2)
 *         bq = ((Sp << 14) - aq Sg) / N;  SA, SB = the box sums of aq, bq
 *         t  = clamp((SA g + SB + (N << 13)) / (N << 14), 0, 255)
 *   tt  = max(t, tq); J_c = clamp(A_c + ((I_c - A_c) 510 + tt) / (2 tt), 0, 255)
 * Normalised parameters: patch odd in 3..31; wq = omega in 1/256, 1..256;
 * tq = t_min in 1/255, 1..255; radius 0..64; eq = eps 65025, 1..2^20.
 * H * W <= 2^24 (the per-level channel sums are 32-bit).  in and out may not
 * alias.  air_out (nullable): {A_b, A_g, A_r, L, cnt} per frame; t_out
 * (nullable): the B x H x W plane of t.  ws: 16-byte aligned. */
size_t rv_dcp_ws_bytes(int B, int H, int W, int radius);
int rv_dcp_dehaze_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                     int patch, int wq, int tq, int radius, int eq, void* ws,
                     size_t ws_bytes, int32_t* air_out, uint8_t* t_out, void* stream);

/* Directional rain-streak removal (no reference counterpart: the stronger
 * derain the reference's plugin registry leaves room for; its MedianDerain
 * blurs every pixel to remove a 1-pixel streak).  Integer arithmetic end to
 * end, every division a floor division, every window clipped to the frame
 * (samples outside it are ignored).  With
 *   g        = the gray of rv_gray_span_u8
 *   hmin_k, hmax_k = min / max over the columns x - k/2 .. x + k/2 of the row
 *   o_j      = sgn(j slant) ((|j slant| + 2) >> 2), so o_-j = -o_j
 *   emin_n(P)(y, x) = min of P(y + j, x + o_j) over j in [-n/2, n/2];
 *   emax_n likewise with max; open_n = emax_n . emin_n
 * the op is
 *   T0 = g - hmax_w(hmin_w(g))   (bright runs narrower than w; >= 0)
 *   T  = T0 >= thr ? T0 : 0
 *   S  = min(T, open_L(hmax_3(T)))   (at least L rows long along the slant)
 *   M > 0: R = hmax_9(open_M(hmax_9(T))); S = 0 where R > 0
 *          (structures at least M long, lane markings and poles, are kept;
 *          9 = RV_STREAK_REJECT_W)
 *   den = max(1, 255 - g); out_c = max(0, I_c - (S (255 - I_c) + (den >> 1)) / den)
 *          (the inverse of I' = I + (255 - I) a; out = in where S = 0)
 * Normalised parameters: w = width odd in 3..15; L = min_len odd in 3..33;
 * M = max_len 0 (off) or odd with L < M <= 97; slant -4..4 in quarter pixels
 * of x per row; thr 1..255.  B <= 65535.  in and out may not alias.  s_out
 * (nullable): the B x H x W plane of S.  ws: 16-byte aligned, two planes of
 * B x H x (W rounded up to 16) bytes, four with max_len > 0. */
#define RV_STREAK_REJECT_W 9
size_t rv_streak_ws_bytes(int B, int H, int W, int max_len);
int rv_streak_derain_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                        int width, int min_len, int max_len, int slant, int thr, void* ws,
                        size_t ws_bytes, uint8_t* s_out, void* stream);

/* PreprocessPipeline.__call__ (src/preprocess/pipeline.py:32-45) of any
 * chain of the built-in ops, followed by the detector's LetterBox
 * (src/detect/yolo_ultralytics.py:28-35), as stream-ordered launches only:
 * no allocation, no host read of device data, no synchronisation.
 *
 * The chain is a fixed-size host descriptor read at call time (a launch
 * schedule copies it by value, like geo).  Per frame:
 *   !enabled or n_ops == 0                      -> proc = raw
 *   gate_on and not (double)span < thresh       -> proc = raw
 *     (span = rv_gray_span_u8's max - min of BGR2GRAY; pipeline.py:24-30,37-40)
 *   else                                        -> proc = ops applied in order
 * then lb = LetterBox(proc).  Ops may repeat and come in any order; their
 * parameters are the normalised ones (clahe_dehaze.py:14-17: tiles =
 * max(2, tile_grid); median_derain.py:11-13: k odd in [3, 9]). */
#define RV_CHAIN_CLAHE 0
#define RV_CHAIN_MEDIAN 1
#define RV_CHAIN_DCP 2
#define RV_CHAIN_STREAK 4 /* kind 3 is not defined and is refused */
#define RV_CHAIN_YCRCB 0
#define RV_CHAIN_LAB 1
#define RV_CHAIN_MAX_OPS 4
/* One op in 24 bytes.  A DCP op (rv_dcp_dehaze_u8's normalised parameters)
 * keeps {kind, tq, radius, patch} in the four ints and {wq, eq} in the bytes
 * of `clip`; never fused with a neighbour, its chain runs op by op.  A streak
 * op (rv_streak_derain_u8's normalised parameters) keeps {kind, thr, min_len,
 * width} in the four ints and {max_len, slant} in the bytes of `clip`, and is
 * a pass of its own in the same way. */
typedef struct rv_chain_op {
  int32_t kind; /* RV_CHAIN_CLAHE / RV_CHAIN_MEDIAN / RV_CHAIN_DCP / RV_CHAIN_STREAK */
  union {
    int32_t space; /* CLAHE: RV_CHAIN_YCRCB / RV_CHAIN_LAB */
    int32_t tq;    /* DCP: 1..255 */
    int32_t thr;   /* streak: 1..255 */
  };
  union {
    int32_t tiles;  /* CLAHE: grid, 2..64 */
    int32_t radius; /* DCP: 0..64 */
    int32_t min_len; /* streak: odd, 3..33 */
  };
  union {
    int32_t k;     /* median: 3, 5, 7 or 9 */
    int32_t patch; /* DCP: odd, 3..31 */
    int32_t width; /* streak: odd, 3..15 */
  };
  union {
    double clip; /* CLAHE: clipLimit */
    struct {
      int32_t wq; /* DCP: 1..256 */
      int32_t eq; /* DCP: 1..2^20 */
    };
    struct {
      int32_t max_len; /* streak: 0, or odd in min_len + 2..97 */
      int32_t slant;   /* streak: -4..4 */
    };
  };
} rv_chain_op;
typedef struct rv_chain_desc {
  int32_t enabled; /* preprocess.enabled */
  int32_t n_ops;   /* 0..RV_CHAIN_MAX_OPS */
  int32_t gate_on; /* auto_gate.enable_low_contrast_gate */
  int32_t reserved;
  double contrast_thresh; /* auto_gate.contrast_thresh */
  rv_chain_op ops[RV_CHAIN_MAX_OPS];
} rv_chain_desc;
#define RV_CHAIN_DESC_BYTES 120 /* sizeof(rv_chain_desc) */

/* How rv_preprocess_chain_u8 runs a configuration (host only, no GPU):
 * RV_CHAIN_ROUTE_FUSED: [CLAHE(YCrCb), median 3], gate off, in the fused
 *   CLAHE + median (+ letterbox) pass: the launches of
 *   rv_clahe_median_letterbox_u8 (rv_clahe_median_u8 when geo is NULL);
 * RV_CHAIN_ROUTE_FUSED_GATED: the same chain with the gate on: three small
 *   gate launches, then the same single pass in which a passed frame's
 *   blocks copy raw to proc and letterbox raw;
 * RV_CHAIN_ROUTE_OPS: everything else, op by op (adjacent CLAHE(YCrCb) +
 *   median fused where rv_clahe_median_fits), ping-pong between `out` and
 *   one scratch batch, then rv_letterbox_u8's kernel.
 * geo (nullable: no letterbox wanted) as rv_letterbox_geometry writes it.
 * RV_EINVAL for a bad descriptor. */
#define RV_CHAIN_ROUTE_FUSED 0
#define RV_CHAIN_ROUTE_FUSED_GATED 1
#define RV_CHAIN_ROUTE_OPS 2
int rv_preprocess_chain_route(const rv_chain_desc* desc, int H, int W, const int* geo);
/* Workspace bytes for B frames of H x W with `pitch` bytes per row: the gate's
 * 2*B ints + B flags, the largest op's LUTs, and one scratch batch
 * (B*H*pitch) when the chain runs as two or more passes, and
 * rv_dcp_ws_bytes of the largest radius when it holds a DCP op, and
 * rv_streak_ws_bytes of the largest max_len when it holds a streak op.  0 for a bad
 * descriptor or shape (and when nothing is needed). */
size_t rv_preprocess_chain_ws_bytes(const rv_chain_desc* desc, int B, int H, int W, int pitch);
/* in -> out (proc) and, when lb_out and geo are both given, the letterbox
 * of proc -> lb_out (B x geo[0] x geo[1] x 3).  in, out and ws may not
 * alias.  out may be NULL for a disabled or empty chain ("proc is the
 * input": only the letterbox is produced).  A LAB op needs rv_lab_init() on the device beforehand when the
 * call must not synchronise (a recorded schedule). */
int rv_preprocess_chain_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                           const rv_chain_desc* desc, void* ws, size_t ws_bytes,
                           uint8_t* lb_out, const int* geo, void* stream);

/* ------------------------------------------------------------------------ */
/* Detect: YOLOUltralytics (src/detect/yolo_ultralytics.py:26-53).           */
/* ------------------------------------------------------------------------ */

/* Ultralytics LetterBox(640, auto=True, stride=32) geometry for an H x W
 * frame: writes {out_h, out_w, new_h, new_w, top, left} into geo[6]. */
int rv_letterbox_geometry(int H, int W, int imgsz, int stride, int* geo);

/* LetterBox pixels: cv2.resize(INTER_LINEAR, 8U fixed point) to new_h x
 * new_w, then cv2.copyMakeBorder(top, ., left, ., BORDER_CONSTANT, 114).
 * Output is BGR u8, B x out_h x out_w x 3, tightly packed. */
int rv_letterbox_u8(const uint8_t* in, uint8_t* out, int B, int H, int W,
                    int pitch, const int* geo, void* stream);


/* --- YOLOv8 / YOLOv5u model (the Ultralytics graph run by model.predict,
 * yolo_ultralytics.py:16-35).  variant: 0=n 1=s 2=m 3=l 4=x (yolov8.yaml
 * scales: Conv / C2f / SPPF / Detect at model.22); 5=n 6=s 7=m 8=l 9=x of
 * YOLOv5u (yolov5.yaml scales: Conv k6 / C3 / SPPF under the same Detect at
 * model.24 -- the anchor-free "u" checkpoints yolov5n.pt ... resolve to).
 * Every entry that takes a variant accepts 0..9; YOLOv5u plans are bf16 only
 * (RV_YOLO_DTYPE_FP8 with a variant >= 5: RV_EINVAL), class counts 1..128 as
 * for YOLOv8.  YOLOv5u's model.0 is a 6x6 stride-2 pad-2 conv on the u8
 * letterbox (in_h, in_w multiples of 32, so its map is in_h/2 x in_w/2): it
 * runs on i8 MFMAs with exact integer sums under the contract of the 3x3
 * first conv -- f64 weights w[o][2-ch][ky][kx] / 255 as integers at 2^-23 of
 * the channel's largest magnitude, three balanced base-256 digits, the value
 * s (65536 T0 + (256 T1 + T2)) + b in f32 -- within 1 bf16 ulp of the f64
 * conv; out-of-image taps are the conv's zero padding.
 * Weights are BN-fused conv weights + biases in Ultralytics
 * state_dict order (rv_yolo_conv_info), flattened as, per conv,
 * weight[cout][cin][k][k] then bias[cout] (f32). */
int rv_yolo_num_convs(int variant);
/* info[5] = {cin, cout, k, stride, silu}; name = "model.2.m.0.cv1" etc. */
int rv_yolo_conv_info(int variant, int idx, int* info, char* name, int name_cap);
size_t rv_yolo_flat_floats(int variant);
size_t rv_yolo_packed_bytes(int variant);
/* Host-side packer: flat f32 -> device layout (bf16 [Cout16][ky][kx][Cin32],
 * f32 biases); the caller copies host_out to device memory it owns. */
int rv_yolo_pack(int variant, const float* flat, size_t n, void* host_out, size_t out_bytes);
/* Plan a model for in_h x in_w letterboxed inputs (multiples of 32) and up
 * to max_B images; dev_packed must stay valid for the handle's lifetime. */
int rv_yolo_create(int variant, const void* dev_packed, int max_B, int in_h, int in_w,
                   void** handle);
int rv_yolo_destroy(void* handle);
/* Handle options.  RV_YOLO_OPT_RAW_UNFUSED (default 1): a forward asked for
 * raw_out runs the unfused stem, so the P1 map (X0) lands in the workspace
 * for layer-wise inspection (and the C2f blocks unfused); 0: raw forwards
 * run the production kernel sequence, so raw_out is what the candidate
 * path computed. */
#define RV_YOLO_OPT_RAW_UNFUSED 1
/* RV_YOLO_OPT_FUSE_C2F: the narrow C2f blocks run as cv1 + one fused launch
 * for the bottlenecks and cv2 (bit-identical to the unfused convs): 1
 * (default) the hidden-width-16 blocks (YOLOv8n model.2), 2 also the
 * width-32 ones (model.4 / model.15; measured slower than unfused), 0 none:
 * one launch per conv. */
#define RV_YOLO_OPT_FUSE_C2F 2
/* RV_YOLO_OPT_STEM_X1 (default 0): the fused stem (conv0 + model.1, and
 * model.2.cv1 from its registers) also writes the X1 map; by default X1
 * never reaches HBM when model.2.cv1 is fused. */
#define RV_YOLO_OPT_STEM_X1 3
/* RV_YOLO_OPT_HEAD_STREAMS (default 1): the P3 / P4 Detect heads run on two
 * side streams of the handle (forked / joined with events) so they overlap
 * the rest of the neck; 0 keeps them on the caller's stream (a pipelined
 * caller whose stages already overlap). */
#define RV_YOLO_OPT_HEAD_STREAMS 4
/* RV_YOLO_OPT_FUSE_CV1 (default 1): model.3 and model.4.cv1 (the C2f's
 * first 1x1) run as one launch -- the 1x1 works on model.3's output tile in
 * LDS, so that map never reaches HBM; bit-identical to the two launches.
 * Raw parity forwards with RV_YOLO_OPT_RAW_UNFUSED keep them separate. */
#define RV_YOLO_OPT_FUSE_CV1 5
/* Option 6 (the chained Detect head) is retired and must not be reused. */
/* RV_YOLO_OPT_C2F_TAP_PAIRS (default 1): the fused hidden-width-16 C2f chain
 * (model.2 of YOLOv8n) runs its 3x3 convs on tap pairs -- two taps' 16
 * channels per 32-deep MFMA k-step, 5 k-steps instead of 9 half-zero ones;
 * the sums round differently (within 1 bf16 ulp of the per-tap order).
 * 0: the per-tap k order, bit-identical to the unfused launches. */
#define RV_YOLO_OPT_C2F_TAP_PAIRS 7
/* RV_YOLO_OPT_HEAD_SPARSE (default 2): the sparse Detect head.  The decode
 * runs the class branch alone and lists the candidates (best class score >
 * conf); the box branch behind model.22.cv2.i.0 -- cv2.i.1, cv2.i.2, DFL,
 * dist2bbox -- then runs at the candidates only, each from the 3x3
 * neighbourhood of cv2.i.0's map, instead of densely over every anchor.
 * Candidate rows, counts and order are bit-identical to the dense head.
 * 0: dense.  1: sparse wherever the head has the form (a bf16 plan whose
 * decode would take form 2 of rv_yolo_head_form, and a candidate list is
 * asked for); other forwards -- raw_out, fp8, wider heads -- stay dense.
 * 2: auto, sparse as under 1 when the call's conf >= 0.1 and B >= 8.  Other
 * values: RV_EINVAL.  The sparse kernel is correct at any candidate count,
 * only slower than the dense convs once most anchors are candidates. */
#define RV_YOLO_OPT_HEAD_SPARSE 8
/* RV_YOLO_OPT_STEM6_FUSED: YOLOv5nu (C0 = 16, c2 = 32) runs model.0 (k6) and
 * model.1 as one kernel with the P1 map in LDS; X1 is bit-identical to the
 * two launches'.  Raw parity forwards with RV_YOLO_OPT_RAW_UNFUSED run the
 * two launches.  0: always two launches.  No effect on other plans. */
#define RV_YOLO_OPT_STEM6_FUSED 9

/* One bf16 NHWC conv through the detector's conv launcher (layer tests;
 * the building block behind rv_yolo_forward, which the reference's
 * model.predict call replaces, src/detect/yolo_ultralytics.py:28-35):
 * k in {1, 3} (pad k / 2), stride 1 or 2, bias, SiLU when act != 0, plus an
 * optional bf16 residual view of the output's shape.  w: packed
 * [Cout_pad16][k*k][Cin_pad32] bf16, bias: f32 [Cout_pad16].  cfg6
 * (nullable): {MR, NR, G, resw, persist, kind} as rv_yolo_tuned_config
 * reports; RV_EINVAL when it is not valid for the layer.
 *
 * in / out / res may be channel slices of wider NHWC tensors: the pointer
 * is the slice's first channel of pixel 0 and in_cs / out_cs / res_cs the
 * wide tensor's channel count (elements per pixel).  Supported, and checked
 * before anything is launched (RV_EINVAL otherwise, nothing written):
 *   - input side, read with 16-byte loads of 8 channels: Cin % 8 == 0,
 *     in_cs % 8 == 0, `in` 16-byte aligned (a slice offset of whole 8
 *     channels).  Only channels [0, Cin) of the view are read, so whatever
 *     the wide tensor's other channels hold (NaN included) has no effect;
 *   - output side, written with 8-byte stores of 4 channels (16-byte stores
 *     of 8 where Cout % 16 == 0, at 8-byte alignment): Cout % 4 == 0,
 *     out_cs % 4 == 0, `out` 8-byte aligned (a slice offset of whole 4
 *     channels).  Only channels [0, Cout) of the view are written;
 *   - residual, read with 8-byte loads of 4 channels: res_cs % 4 == 0, `res`
 *     8-byte aligned; it must not overlap the channels the call writes;
 *   - w and bias 16-byte aligned, padded as above (rows >= Cout and input
 *     channels >= Cin of w zero);
 *   - B * Hin * Win * in_cs, * out_cs and * res_cs each below 2^31.
 * A 1x1 stride-2 conv has no LDS-staged configuration (every cfg6 is
 * rejected for it) and runs the generic kernel. */
int rv_conv_bf16(const void* in, int B, int Hin, int Win, int Cin, int in_cs, const void* w,
                 const float* bias, int Cout, int k, int stride, void* out, int out_cs,
                 const void* res, int res_cs, int act, const int* cfg6, void* stream);
int rv_yolo_set_option(void* handle, int opt, int value);

/* --- YOLO11 (yolo11.yaml: Conv / C3k2 / SPPF / C2PSA, Detect at model.23
 * with a depthwise-separable class branch).  variant: 20=n 21=s 22=m 23=l
 * 24=x.  Variants 10..19 are no variant: every entry returns RV_EINVAL (the
 * size_t entries 0) for them.  YOLO11 plans are bf16 only (RV_YOLO_DTYPE_FP8
 * with a variant >= 20: RV_EINVAL), class counts 1..128 as for YOLOv8.  The
 * first conv is YOLOv8's (k3 s2 on i8 MFMAs).  The Detect head is dense only:
 * RV_YOLO_OPT_HEAD_SPARSE has no effect on these plans and rv_yolo_head_form
 * never reports 3 for them; no launch of a YOLO11 forward is fused.
 *
 * A depthwise conv (the class branch's DWConv 3x3, the attention's `pe`) is a
 * conv of the list like any other: rv_yolo_conv_info reports cin = cout = C,
 * its flat weights are the state_dict's [C][1][3][3] then bias[C], and
 * rv_yolo_conv_groups returns C for it (1 for a dense conv; RV_EINVAL for a
 * bad variant / nc / index).  Packed: bf16 [ky * 3 + kx][C_pad8], f32 bias. */
int rv_yolo_conv_groups(int variant, int nc, int idx);

/* One depthwise 3x3 conv (stride 1, zero pad 1) on bf16 NHWC maps: per
 * channel c, out = act(bias[c] + sum w[ky * 3 + kx][c] in[y + ky - 1][x + kx - 1][c])
 * (+ res), f32 accumulation in the order bias, ky 0..2, kx 0..2 inside, SiLU
 * when act != 0, the optional bf16 residual added after the activation, one
 * rounding to bf16.  w: bf16 [9][C], bias: f32 [C].
 *
 * in / out / res are views (pointer to pixel 0 of the wide tensor, its
 * channel count *_cs, the view's first channel *_co).  The input view may be
 * grouped: with in_gw > 0, logical channel c is channel in_co + (c / in_gw) *
 * in_gs + c % in_gw of the wide tensor (the v part of a qkv map: in_gw 64,
 * in_gs 128, in_co 64); in_gw = in_gs = 0: channels [in_co, in_co + C).
 * Checked before anything is launched (RV_EINVAL otherwise, nothing written):
 * C a positive multiple of 8; every *_cs, *_co, in_gw, in_gs a multiple of 8
 * and every pointer 16-byte aligned (16-byte accesses of 8 channels); C %
 * in_gw == 0, in_gs >= in_gw; each view's channels inside its *_cs; B and
 * ceil(H / 8) at most 65535.  Only the view's channels are read or written. */
int rv_dwconv3x3_bf16(const void* in, int B, int H, int W, int C, int in_cs, int in_co, int in_gw,
                      int in_gs, const void* w, const float* bias, void* out, int out_cs,
                      int out_co, const void* res, int res_cs, int res_co, int act, void* stream);

/* Multi-head self-attention of a PSA block (key_dim 32, head_dim 64) over the
 * N positions of each of B images, all images and heads in one launch.  qkv:
 * bf16 view of B * N rows of qkv_cs channels; head h reads channels qkv_co +
 * 128 h + [0, 32) as q, [32, 64) as k, [64, 128) as v.  Per image and head
 * S = q^T k * 32^-1/2 in f32 (the scale multiplies the f32 scores), the row
 * maximum is subtracted, P = softmax over the keys (f32 denominator, P
 * rounded to bf16 only as the P v operand), o = P v written as bf16 to channel
 * out_co + 64 h + d of the output view (B * N rows of out_cs channels).  One
 * code path for every N: 32-key tiles with online rescaling, tail keys
 * masked.  Checked before anything is launched (RV_EINVAL otherwise, nothing
 * written): B, N, heads >= 1 (B, heads <= 65535); qkv_co + 128 heads <=
 * qkv_cs, out_co + 64 heads <= out_cs; qkv_cs, qkv_co multiples of 8 and qkv
 * 16-byte aligned; out_cs, out_co multiples of 4 and out 8-byte aligned.
 * Nothing outside those rows and channels is read or written. */
int rv_psa_attention_bf16(const void* qkv, int B, int N, int heads, int qkv_cs, int qkv_co,
                          void* out, int out_cs, int out_co, void* stream);

/* fp8 plans (BASELINE configs[4]: "YOLOv8m 1280x1280 fp8 MFMA conv path").
 * dtype RV_YOLO_DTYPE_FP8: every conv except conv 0 (f32 weights, u8 input)
 * and the Detect head's last 1x1 stage (bf16, inside the decode) runs on
 * v_mfma_f32_16x16x32_fp8_fp8 with OCP e4m3fn weights (per output channel
 * power-of-two scale, round to nearest even, saturated at 448) and e4m3
 * activations (one power-of-two scale per activation buffer, value = code *
 * scale, set with rv_yolo_set_act_scales before the first forward; the
 * head's .1 stage writes bf16 features for the decode).  Packed layout per
 * fp8 conv: e4m3 [Cout16][ky][kx][Cin64], f32 bias [Cout16], f32 weight
 * scales [Cout16].  dtype RV_YOLO_DTYPE_BF16 = rv_yolo_pack / rv_yolo_create. */
#define RV_YOLO_DTYPE_BF16 0
#define RV_YOLO_DTYPE_FP8 1
size_t rv_yolo_packed_bytes2(int variant, int dtype);
int rv_yolo_pack2(int variant, int dtype, const float* flat, size_t n, void* host_out,
                  size_t out_bytes);
int rv_yolo_create2(int variant, int dtype, const void* dev_packed, int max_B, int in_h, int in_w,
                    void** handle);

/* Custom class counts (a YOLOv8 fine-tuned on nc classes; the reference takes
 * nc from the checkpoint, src/detect/yolo_ultralytics.py:16-24).  Every entry
 * above that takes no nc means nc = 80 and is unchanged.  1 <= nc <= 128 (the
 * NMS class mask is 4 x 32 bits); outside it the call returns RV_EINVAL (the
 * size_t entries 0), rv_last_error names the range and nothing is written.
 * fp8 plans exist for nc = 80 only: rv_yolo_pack3 / rv_yolo_create3 refuse
 * RV_YOLO_DTYPE_FP8 with another nc (RV_EINVAL).
 *
 * Shapes: rv_yolo_conv_info_nc and the flat layout are the Ultralytics
 * state_dict's own: the Detect class branch is c3d = max(h15, min(nc, 100))
 * wide (h15: the P3 width of the variant) and model.22.cv3.i.2 maps c3d -> nc.
 * Padding contract (internal, visible only through the introspection
 * entries): the plan runs the class branch padded to a multiple of 8
 * channels -- the "DA<i>" / "DB<i>" buffers are c2d + pad8(c3d) wide -- and
 * the f32 logits buffers "HD<i>" have rows of pad4(64 + nc) floats.  The
 * packed rows / columns behind the padding are zero, so every padding channel
 * of those buffers is exactly 0 after a forward and every logical channel is
 * the sum it would be without padding.  nc itself is exact everywhere else:
 * raw_out is (B, 4 + nc, A) dense, candidate classes are < nc. */
int rv_yolo_num_convs_nc(int variant, int nc);
int rv_yolo_conv_info_nc(int variant, int nc, int idx, int* info, char* name, int name_cap);
size_t rv_yolo_flat_floats_nc(int variant, int nc);
size_t rv_yolo_packed_bytes3(int variant, int dtype, int nc);
int rv_yolo_pack3(int variant, int dtype, int nc, const float* flat, size_t n, void* host_out,
                  size_t out_bytes);
int rv_yolo_create3(int variant, int dtype, int nc, const void* dev_packed, int max_B, int in_h,
                    int in_w, void** handle);
int rv_yolo_num_classes(void* handle);
/* Decode form of the handle's last forward that ran the decode (-1 before
 * one): 0 = unfused last head stage, f32 logits read from HBM; 1 = last stage
 * fused into the decode, class scan over the logits tile in LDS (any plan;
 * always with raw_out); 2 = fused with the class scores kept in registers
 * (YOLOv8n, nc = 80 or nc <= 64, no raw_out); 3 = form 2 with the class
 * branch only, followed by the sparse box-branch kernel
 * (RV_YOLO_OPT_HEAD_SPARSE).  For tests that must prove which kernel ran. */
int rv_yolo_head_form(void* handle);
/* scales[n]: one per activation buffer (n = rv_yolo_num_buffers; entries of
 * bf16 / f32 buffers are ignored), each a positive power of two. */
int rv_yolo_set_act_scales(void* handle, const float* scales, int n);
/* Per activation buffer: element bytes (1 fp8, 2 bf16, 4 f32), and its name
 * in the plan ("X0", "C2", "CAT14", "SP", "DA0", "model.2.m.0", ...: the
 * tensor or concat it holds; the fp8 oracle keys its scales by these). */
int rv_yolo_buffer_esize(void* handle, int buf);
int rv_yolo_buffer_name(void* handle, int buf, char* name, int cap);
/* The power-of-two scale for a tensor of absolute maximum amax (the rule the
 * packer and calibration use). */
float rv_fp8_scale(double amax);
size_t rv_yolo_ws_bytes(void* handle, int B);
int rv_yolo_num_anchors(void* handle);
/* Forward on B letterboxed u8 BGR images (B x in_h x in_w x 3).  raw_out
 * (nullable): the reference's raw prediction (B, 4+nc, A) f32 = cat(xywh *
 * stride, sigmoid(cls)).  cand (nullable): NMS candidate rows
 * {x1,y1,x2,y2,score,cls,anchor,pad} (32 B) of every anchor whose best class
 * score > conf, in the SEGMENTED layout: per image cand_cap rows, segment j
 * (64 consecutive anchors of one head level, nseg = rv_yolo_cand_segments)
 * owns rows [64 j, 64 j + cand_n[b * nseg + j]) in anchor order; cand_cap
 * >= 64 * nseg.  No atomics, no pre-zeroing. */
int rv_yolo_cand_segments(void* handle);
int rv_yolo_forward(void* handle, const uint8_t* lb, int B, void* ws, size_t ws_bytes,
                    float* raw_out, float conf, void* cand, int cand_cap, int* cand_n,
                    void* stream);
/* The forward in two parts: part 1 = stem .. model.15 (lb used), part 2 =
 * the bottom-up neck, the Detect heads and the decode (lb unused; reads part
 * 1's activations from the same workspace; cand / raw as above; raw_out
 * only with part 0 = the whole forward).  Part 2 needs a part 0 or part 1
 * forward of the same handle before it (launch numbering of the autotuned
 * configurations).  With two handles + workspaces a pipelined caller runs
 * part 2 of step j-1 beside part 1 of step j.  Part 1 itself may run as
 * part 3 (the stem and model.2, lb used) then part 4 (model.3 .. model.15,
 * lb unused; it must continue the handle's last part 3 with the same B and
 * workspace), so a caller can order other work after the stem. */
int rv_yolo_forward_part(void* handle, const uint8_t* lb, int B, void* ws, size_t ws_bytes,
                         float* raw_out, float conf, void* cand, int cand_cap, int* cand_n,
                         void* stream, int part);

/* Introspection for layer-wise parity tests: activation buffers (NHWC,
 * info = {H, W, C, is_f32}, byte offset inside the workspace for batch B)
 * and the conv launches of the last forward (24 ints each: conv index,
 * input view {buf, cs, co, Hin, Win}, Ho, Wo, two output views {buf, cs, co,
 * upsample}, residual view {buf, cs, co}, then a 1x1 conv's virtual concat
 * input {in_up, in2 buf, in2 cs, in2 co, split}: channels [0, split) are the
 * input view's (read upsampled 2x when in_up), the rest in2's; in2 buf -1:
 * none).  Returns the record count. */
int rv_yolo_num_buffers(void* handle);
int rv_yolo_buffer_info(void* handle, int B, int buf, int* info, size_t* off_bytes);
int rv_yolo_trace(void* handle, int* recs, int max_recs);
/* YOLO11 plans: a depthwise conv appears in rv_yolo_trace as a conv; its
 * virtual-concat fields carry the input view's group form instead (in2 buf
 * -1, in2 cs = group stride, split = group width; both 0: contiguous
 * channels) -- attn.pe reads v of its qkv map as {co 64, width 64, stride
 * 128}.  The attention launches of the last forward are reported here, 9 ints
 * each in launch order: qkv view {buf, cs, co}, heads, H, W, output view {buf,
 * cs, co} (rv_psa_attention_bf16 over N = H * W).  Returns the record count
 * (0 for the other families).  Depthwise and attention launches keep a launch
 * index of their own: rv_yolo_conv_candidates reports 0 configurations for
 * them, the autotuner skips them, and rv_yolo_profile times them in their
 * index's slot (an attention under its block's attn.qkv conv index). */
int rv_yolo_attn_trace(void* handle, int* recs, int max_recs);

/* Live device timing of the conv launches (HIP events recorded on the launch
 * stream around every conv_mfma launch of the next max_forwards forwards;
 * 0 disables).  rv_yolo_profile_read synchronises on the events and returns,
 * per conv launch index, the summed ms over the recorded forwards, the
 * algorithmic FLOPs of one launch (2*M*N*K) and the conv index. */
int rv_yolo_profile(void* handle, int max_forwards);
/* The same with every profiled conv launched `reps` times back to back
 * between its event pair (same inputs and output); profile_read then
 * reports the time of ONE launch, free of the per-event dispatch gap. */
int rv_yolo_profile_reps(void* handle, int max_forwards, int reps);
int rv_yolo_profile_read(void* handle, double* ms, double* flops, int* conv, int n);
/* Algorithmic HBM bytes of one launch per conv launch index (inputs read
 * once, outputs written, residual, weights); returns the entries written. */
int rv_yolo_profile_bytes(void* handle, double* bytes, int n);
/* [start, end) in ms of every recorded conv launch of `handle`, after the
 * first recorded event of handle `ref` (same device clock), so the launches
 * of several forward contexts merge into the conv family's chip-wide busy
 * time.  Writes at most n pairs; returns the interval count. */
int rv_yolo_profile_times(void* handle, void* ref, double* t0, double* t1, int n);

/* Per-layer autotuning of the conv kernels (no reference counterpart: it
 * picks, per conv launch of this handle's forward, the fastest of the valid
 * LDS-staged kernel configurations on the given letterboxed batch; later
 * forwards use the choices).  Synchronous, not graph-capturable; call once
 * after rv_yolo_create.  verify != 0: every configuration's output is also
 * compared with the default's (they are bit-identical by construction) and
 * *n_bad counts the ones that were not.  reps: timed launches per config. */
int rv_yolo_autotune(void* handle, const uint8_t* lb, int B, void* ws, size_t ws_bytes,
                     int reps, int verify, int* n_bad, void* stream);
/* cfg6 = {MR, NR, G, resw, persist, kind} of conv launch idx (kind 0: LDS-staged
 * patch kernel, 1: direct-B 1x1 kernel; MR 0 = default
 * heuristic); returns the number of tuned launches (0 before autotuning). */
int rv_yolo_tuned_config(void* handle, int idx, int* cfg6);
/* Install a saved configuration (cfg6 as above) for conv launch idx of a
 * plan with n launches (e.g. reloaded from a file written after an earlier
 * autotune), so a run can skip the autotuner; an invalid entry falls back to
 * the default heuristic at launch. */
int rv_yolo_set_tuned(void* handle, int n, int idx, const int* cfg6);
/* The valid configurations of conv launch idx of the last whole forward
 * (cfg6 entries as above, at most cap written); returns the count (0 for a
 * fused C2f launch). */
int rv_yolo_conv_candidates(void* handle, int idx, int* cfg6, int cap);

/* --- Ultralytics non_max_suppression + scale_boxes + class filter
 * (yolo_ultralytics.py:28-53), one workgroup per image. */
size_t rv_nms_smem_bytes(void);
/* cand / seg_n: the segmented candidate layout of rv_yolo_forward (nseg
 * segments of 64 rows, cap <= 65536 rows per image).  Every candidate is
 * sorted (score desc, anchor asc); only the first max_nms of them enter the
 * greedy pass (Ultralytics non_max_suppression's max_nms = 30000: top
 * max_nms by score).  seg_n[b * nseg + j] rows of segment j are used, from
 * its first slot on; a count outside [0, 64] is clamped to that range, and
 * rows past the count are never read.  Ties in score resolve by the rows'
 * anchor field (< 65536, distinct within an image), not by the slot.
 * iou: the largest f32 not above the reference's double threshold -- the
 * kernel suppresses on (double)ovr > (double)iou with an f32 ovr, which then
 * equals torchvision's `ovr > iou_threshold` for every double threshold
 * (the nearest f32 of 0.6 or 0.3 lies above the double and would keep a pair
 * whose IoU is exactly that f32).  scale5 = {gain (f32 of the python gain), pad_x, pad_y,
 * clip_w, clip_h}; keep_mask4 (nullable = keep all): 128-bit class mask
 * (classes_keep); out: B x max_det x 6 {x1,y1,x2,y2,conf,cls} in score
 * order, out_n[B]; cand_total (nullable): candidates per image before
 * max_nms; ws: rv_nms_ws_bytes(B) bytes of device workspace. */
int rv_nms_postprocess(const void* cand, const int* seg_n, int B, int cap, int nseg,
                       float iou, int max_det, int max_nms, float max_wh, const float* scale5,
                       const uint32_t* keep_mask4, float* out, int* out_n, int* cand_total,
                       void* ws, size_t ws_bytes, void* stream);
/* Device workspace rv_nms_postprocess needs for B images (sort keys of
 * images with more than 4096 candidates: 65536 x 8 B per image). */
size_t rv_nms_ws_bytes(int B);
/* Segments of 64 anchors for a raw prediction with A anchors. */
int rv_cand_segments(int A);
/* Candidate rows from a reference-layout raw prediction (B, 4+nc, A), in the
 * segmented layout (segment j = anchors [64 j, 64 j + 64)); cap >= 64 *
 * rv_cand_segments(A). */
int rv_candidates_from_raw(const float* raw, int B, int nc, int A, float conf, void* cand,
                           int cap, int* seg_n, void* stream);

/* ------------------------------------------------------------------------ */
/* Track: SortTracker.update (src/track/sort_tracker.py:212-278) batched over */
/* S independent streams, with GroundProjector metrics (projector.py:13-84). */
/* ------------------------------------------------------------------------ */
size_t rv_sort_state_bytes(int S, int tmax);
size_t rv_sort_ws_bytes(int S, int tmax, int dmax);
/* ByteTrack's second association threshold (Zhang et al., ECCV 2022: the
 * hard-coded 0.5 of BYTE's second matching); not configurable. */
#define RV_BYTE_SECOND_IOU 0.5
/* Host query: byte offsets, inside a workspace of rv_sort_ws_bytes(S, tmax,
 * dmax), of the two regions a BYTE update (params6[5] > 0, below) writes:
 * the kept rows (S x dmax x 6 f32) and the kept counts (S int32).  Both are
 * 256-byte aligned and disjoint from everything else in the workspace, so
 * they hold one update's result until the next update on that workspace.  A
 * plain update (params6[5] == 0) writes neither. */
int rv_sort_kept_layout(int S, int tmax, int dmax, size_t* dets_off, size_t* n_off);
/* Zero the state (no tracks, next_id = 1); synchronises `stream`.  Layout:
 * per-stream headers, list orders (tmax int32 each) and track pools (tmax
 * slots each); a track keeps its slot for life, the reference's list order
 * is the order array. */
int rv_sort_init(void* state, int S, int tmax, void* stream);
/* One frame per stream, three stream-ordered launches (KF predict over every
 * track; one workgroup per stream for _associate + bookkeeping; KF update /
 * new tracks over every detection).  The update runs in place on state_out;
 * pass state_in == state_out (if they differ, state_in is first copied to
 * state_out).  dets: S x dmax x 6 {x1,y1,x2,y2,conf,cls} f32 (post
 * class-filter), dcount[S]; ts[S] seconds.  params6 = {max_staleness,
 * min_hits, iou_threshold, speed_window, max_distance (<0 = None),
 * track_high_thresh (0 = plain SORT; see BYTE below)}.  H9
 * (nullable = no projector): row-major f64 homography; origin2: projector
 * origin (f32).  Outputs per detection (S x dmax): track id (-1 = None),
 * distance_m and speed_kmh (NaN = None); a new track that is dropped in the
 * same frame (max_staleness < 0, or no free slot) still reports its id and
 * its box's distance, as the reference does.  tmax <= 8192 and the association
 * workgroup's LDS (about 41 B x tmax + 28 B x dmax + 32 KB; with BYTE about
 * 42 B x tmax + 33 B x dmax + 32 KB) <= 160 KB.
 *
 * BYTE (params6[5] = track_high_thresh in (0, 1]): ByteTrack's second
 * association on this SORT, in the one-launch (fused) form only.  A row is
 * high iff (double)conf >= track_high_thresh, else low (the caller has
 * removed the rows below its track_low_thresh).  Stage 1: the greedy
 * association of all tracks with the high rows at iou_threshold.  Stage 2:
 * the same greedy loop over the tracks stage 1 left unmatched whose
 * hit_streak was > 0 before this frame and the low rows, at
 * RV_BYTE_SECOND_IOU.  A stage-2 match is an ordinary match.  New tracks come
 * from unmatched high rows only; unmatched low rows are dropped.  The kept
 * rows (every high row and every matched low row, in input order) and their
 * count go to the workspace regions of rv_sort_kept_layout, rows at or beyond
 * the count zero; out_id / out_dist / out_speed are indexed by kept row, and
 * rows at or beyond the count are -1 / NaN / NaN.  dets is not modified.
 * With every row high the results are the plain update's, bit for bit.
 * params6[5] outside [0, 1] or NaN, or > 0 with RV_SORT_FUSED=0 (the
 * three-launch form has no second association): RV_EINVAL.  A recorded
 * schedule carries the mode in the 48-byte copy of params6. */
int rv_sort_update(void* state_in, void* state_out, int S, int tmax, const float* dets,
                   const int* dcount, int dmax, const double* ts, const double* params6,
                   const double* H9, const float* origin2, void* ws, size_t ws_bytes,
                   int* out_id, double* out_dist, double* out_speed, void* stream);
/* Per-stream capacity report (device outputs, S ints each): live tracks T,
 * next track id, and the sticky overflow flag -- 1 once a frame had more
 * surviving + new tracks than tmax; the new tracks that did not fit were dropped
 * (their ids were still handed out), so that stream's ids diverge from the
 * reference's unbounded track list from then on.  next_id_out / overflow_out
 * are nullable. */
int rv_sort_stats(const void* state, int S, int* T_out, int* next_id_out, int* overflow_out,
                  void* stream);
/* Debug/parity export: per track x[7] (f64) and {id, hits, hit_streak, cls}. */
int rv_sort_export(const void* state, int S, int tmax, double* x_out, int* meta, int* T_out,
                   void* stream);

/* --- Per-camera ground projectors.  The reference runs one process per camera,
 * each with its own geometry.projector, and SortTracker.update takes the
 * projector per call (sort_tracker.py:212-278); the entries above project
 * every stream of a batch with one host-side calibration.  The _cams entries
 * read a table in DEVICE memory instead, one entry per stream (stream s uses
 * cams[s]), at the time the kernel runs: a stream-ordered copy into the table
 * recalibrates a camera, and a recorded schedule (rv_sched_*) sees the change
 * on its next run without being recorded again. */
typedef struct rv_cam_proj {
  double H[9];         /* row-major f64 homography (projector.py:69-72) */
  double max_distance; /* < 0: None */
  float origin[2];
  int32_t enabled;     /* 0: this stream's projector is None */
  int32_t reserved;
} rv_cam_proj;
#define RV_CAM_PROJ_BYTES 96 /* sizeof(rv_cam_proj) */
/* rv_sort_update with stream s projected through cams[s] (device, S entries,
 * 8-byte aligned; NULL = no stream has a projector).  params6[4] is ignored:
 * max_distance is the table's.  Everything else as rv_sort_update.
 * Stream s behaves as SortTracker.update(dets, ts, projector_s) with the
 * projector the table holds when the call runs.  After a change the speed
 * history keeps the ground positions it holds, so a speed may span the old
 * and the new calibration (sort_tracker.py:147-168).  While enabled == 0 a
 * matched track skips update_metrics and keeps reporting its last
 * current_distance / current_speed (sort_tracker.py:242-247); a new track
 * reports None.  rv_sort_update does not do the latter: without a projector
 * it writes NaN for every detection. */
int rv_sort_update_cams(void* state_in, void* state_out, int S, int tmax, const float* dets,
                        const int* dcount, int dmax, const double* ts, const double* params6,
                        const rv_cam_proj* cams, void* ws, size_t ws_bytes, int* out_id,
                        double* out_dist, double* out_speed, void* stream);

/* ------------------------------------------------------------------------ */
/* Result hand-back (yolo_ultralytics.py:44-52 `.cpu().numpy()` + Detection  */
/* construction; sort_tracker.py:234-247 fills track_id / distance_m /       */
/* speed_kmh).  One record per step: int32 n[S] (padded to 16 B), then       */
/* S x dmax rows of 48 B {f32 x1,y1,x2,y2,conf; i32 cls, track_id (-1 =      */
/* None), pad; f64 distance_m, speed_kmh (NaN = None)}, rows >= n[s] zeroed. */
/* ------------------------------------------------------------------------ */
size_t rv_results_bytes(int S, int dmax);
/* Packs the NMS rows (S x dmax x 6 f32) + counts and the SORT outputs
 * (track_id / distance_m / speed_kmh, S x dmax; each nullable = None) into
 * dev_stage (>= rv_results_bytes) and, when host_dst is non-null (pinned
 * host memory), copies the record there with one stream-ordered
 * hipMemcpyAsync.  Graph-capturable. */
int rv_results_handback(const float* dets, const int* det_n, const int* track_id,
                        const double* distance_m, const double* speed_kmh, int S, int dmax,
                        void* dev_stage, size_t stage_bytes, void* host_dst, void* stream);

/* --- Standalone pieces of SortTracker.update / GroundProjector, batched over
 * S streams (csrc/track_ops.hip; rv_sort_update fuses the same math). */
/* _iou_matrix (sort_tracker.py:74-80, _iou :55-71) in f32 scalar order.
 * trk: S x Tmax x 4, det: S x Dmax x 4 (x1,y1,x2,y2) f32; T[S], D[S] valid
 * counts (device).  out: S x Tmax x Dmax, zero outside T[s] x D[s]. */
int rv_iou_matrix_batched(const float* trk, const int* T, const float* det, const int* D,
                          float* out, int S, int Tmax, int Dmax, void* stream);
/* _associate's greedy loop (sort_tracker.py:196-208): argmax (first max in
 * row-major order), stop below thr (f64 compare), accept if row and column
 * are free, mask both with -1.  M (S x Tmax x Dmax, e.g. from
 * rv_iou_matrix_batched) is modified in place like the reference's matrix.
 * Outputs (device): match_t / match_d (S x min(Tmax, Dmax)) in acceptance
 * order, n_match[S], trk_match (S x Tmax: det index or -1), det_match
 * (S x Dmax: track index or -1); the reference's unmatched lists are the
 * -1 entries in ascending order.  thr <= -1 (an endless loop in the
 * reference) stops once every row is masked. */
int rv_greedy_assign_batched(float* M, const int* T, const int* D, int S, int Tmax, int Dmax,
                             double thr, int* match_t, int* match_d, int* n_match,
                             int* trk_match, int* det_match, void* stream);
/* GroundProjector.project_bbox + distance (projector.py:30-47, 74-84): foot
 * point (0.5*(x1+x2), y2) through the f64 homography H9 (device, row-major);
 * out_xy (n x 2 f64, NaN = None); out_dist (nullable, n f64, NaN = None):
 * f32 norm to origin2 (device, nullable = no distance), capped at
 * max_distance when >= 0. */
int rv_homography_project_f64(const double* H9, const float* boxes, int n,
                              const float* origin2, double max_distance,
                              double* out_xy, double* out_dist, void* stream);

/* The tracker-off branch of the per-frame loop (main_preview.py:101-109:
 * `tracker is None`): for dets (S x dmax x 6 f32, device) with det_n (S,
 * device) valid rows per stream, out_id = -1 (track_id None), out_speed NaN
 * (speed_kmh None) and out_dist = projector.distance_for_bbox(bbox)
 * (projector.py:49-51; NaN = None) when H9 (host, 3x3 f64 row-major) is
 * given, else NaN.  origin2 (host, 2 f32) is required with H9;
 * max_distance < 0 = no cap.  Every out array is S x dmax, device. */
int rv_untracked_metrics(const float* dets, const int* det_n, int S, int dmax,
                         const double* H9, const float* origin2, double max_distance,
                         int* out_id, double* out_dist, double* out_speed, void* stream);
/* The same with stream s projected through cams[s] (device, S entries, as for
 * rv_sort_update_cams; NULL or enabled == 0: that stream's distances are
 * NaN). */
int rv_untracked_metrics_cams(const float* dets, const int* det_n, int S, int dmax,
                              const rv_cam_proj* cams, int* out_id, double* out_dist,
                              double* out_speed, void* stream);
/* rv_homography_project_f64 over a camera table: box i (boxes: n x 4 f32,
 * device) goes through camera box_cam[i] (device int32, n entries) of cams
 * (device, S entries).  out_xy (n x 2 f64) and out_dist (nullable, n f64) are
 * NaN where that camera is disabled or the projection is None; a box_cam
 * value outside [0, S) gives NaN outputs for that box and reads no entry. */
int rv_homography_project_cams(const rv_cam_proj* cams, int S, const float* boxes,
                               const int* box_cam, int n, double* out_xy, double* out_dist,
                               void* stream);

/* ------------------------------------------------------------------------ */
/* Ingest: NV12 -> BGR (cv2.COLOR_YUV2BGR_NV12, 8U, BT.601 video range,      */
/* 20-bit fixed point).  The device half of a decode front end for           */
/* src/io_video/capture.py:10-24: host-fed NV12 is 1.5 B/pixel over PCIe     */
/* instead of 3.  y: B frames of H x W (y_pitch, y_frame_stride bytes apart); */
/* uv: interleaved U,V, H/2 x W (uv_pitch, uv_frame_stride); H, W even.      */
/* A packed NV12 batch is y = base, uv = base + H*W, both strides H*W*3/2.   */
/* ------------------------------------------------------------------------ */
int rv_nv12_to_bgr_u8(const uint8_t* y, const uint8_t* uv, int y_pitch, int uv_pitch,
                      size_t y_frame_stride, size_t uv_frame_stride, uint8_t* out,
                      int B, int H, int W, int pitch, void* stream);

/* ------------------------------------------------------------------------ */
/* Augment: fog + rain synthetic inputs (EnhancedFogSynthesizer.synthesize,  */
/* src/augment/fog.py:239-299; tools/fog_batch.py:7-34 drives it offline).   */
/* Restated subset: depth proxy, value-noise beta map, transmission, airlight */
/* gradient map, scattering I = J t + A (1 - t), global veil, tint, gamma,    */
/* plus rain streaks.  Parameters are drawn on the host                       */
/* (rvs_amd/augment/fog.py); the OpenCV filters are not restated. */
/* ------------------------------------------------------------------------ */
#define RV_FOG_NCONST 26
#define RV_FOG_NPARAM 16
/* consts (host, RV_FOG_NCONST f32): {vx, vy, dv_max, d_min, d_range, 0,
 *   rain_p, rain_len, n_oct, [gh, gw, amp, 0] x 4 octaves, norm}.
 * scene (device f32, 4*H + W + 3*n_oct*(H + W)): per-row 0.7*dp/dp_max,
 *   depth factor (sky boost x road damp), global-veil weight, airlight
 *   vertical gradient; the per-column airlight horizontal gradient; then per
 *   octave the noise sample taps: rows {y0[H], y1[H], wy[H]}, columns
 *   {x0[W], x1[W], wx[W]} (ys = (y*gh)/H in f32, y0 = floor, y1 = min(y0+1,
 *   gh), wy = ys - y0; the same along x).
 * frame_params (device, B x RV_FOG_NPARAM f32): {beta, A_b, A_g, A_r,
 *   A_scale, tint_b, tint_g, tint_r, gamma, rain_seed (< 2^24), 0...}.
 * grids (device, B x grid_stride f32): per frame, the octaves' value-noise
 *   grids, (gh+1) x (gw+1) each, concatenated.
 * ws: rv_fog_ws_bytes(B) bytes of device scratch (noise min / max). */
size_t rv_fog_ws_bytes(int B);
int rv_fog_rain_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                   const float* consts, int n_consts, const float* scene,
                   const float* frame_params, const float* grids, int grid_stride,
                   void* ws, size_t ws_bytes, void* stream);

/* The whole EnhancedFogSynthesizer.synthesize (fog.py:227-299) with every
 * filter, as opencv-python runs it: the image airlight (band luminance
 * 0.9-quantile, masked mean, tint, filtered gradient map; fog.py:120-139),
 * the edge-guided transmission (_guided_filter's bilateralFilter fallback,
 * d 17, sigma 12 / 12; fog.py:55-67,172-179), scattering + global veil,
 * _glow (fog.py:182-191), _depth_blur (fog.py:194-214),
 * _local_contrast_fade (fog.py:217-224), tint, gamma, sensor noise, rain.
 * consts / scene / grids / rain as rv_fog_rain_u8.
 * full (host, RV_FOG_NFULL f32): {band_h, k, t, edge_guided, 0...}: the
 *   airlight band rows (max(10, int(0.12 H))) and np.quantile's f32 'linear'
 *   constants for n = band_h * W (k = floor((n-1)*0.9f), t = remainder).
 * depth (device f32 H x W): _depth_proxy's clipped depth.
 * amap_unit (device f32 H x W): the airlight filter applied to vgrad x xgrad
 *   (the per-channel map is a_c times it; rvs_amd.augment.airlight_unit_map).
 * bands (device u8 H x W): the _depth_blur band of each pixel (0..2, 3 none).
 * frame_params (device, B x RV_FOG_NPARAM_FULL f32): {beta, airlight tint
 *   b/g/r, airlight target mean, tint b/g/r, gamma, rain_seed, glow strength,
 *   contrast drop, has_noise, band kernel sizes x 3 (0 = skip), glow mask
 *   kernel k, glow image kernel k2, fade diameter d, 0...}; k, k2, band sizes
 *   <= 63, d <= 15.
 * noise (device f32 B x H x W x 3 or NULL): the sensor-noise normals of the
 *   frames whose has_noise is set.
 * ws: rv_fog_full_ws_bytes(B, H, W) bytes (56 B per pixel + partials).
 * H, W >= 64. */
#define RV_FOG_NPARAM_FULL 24
#define RV_FOG_NFULL 8
size_t rv_fog_full_ws_bytes(int B, int H, int W);
int rv_fog_full_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                   const float* consts, int n_consts, const float* full, int n_full,
                   const float* scene, const float* depth, const float* amap_unit,
                   const uint8_t* bands, const float* frame_params, const float* grids,
                   int grid_stride, const float* noise, void* ws, size_t ws_bytes,
                   void* stream);

/* ------------------------------------------------------------------------ */
/* Capture front end (VideoSource, src/io_video/capture.py:10-24; README    */
/* module 8's async pipeline).  One reader thread per source fills a ring of */
/* pinned host slots from a file; frames are stamped with the wall-clock    */
/* time they were read (capture.py:20).  Formats: YUV4MPEG2 4:2:0 (handed   */
/* out as NV12), raw NV12, raw BGR, and Motion-JPEG (baseline JPEG images    */
/* back to back; the reader thread entropy-decodes each into a coefficient   */
/* record, see "Baseline JPEG" below).  No AVI / MP4 demuxer, no H.264, no   */
/* live camera here.                                                        */
/* ------------------------------------------------------------------------ */
#define RV_CAP_Y4M 0
#define RV_CAP_NV12 1
#define RV_CAP_BGR 2
#define RV_CAP_MJPEG 3
/* W, H are read from the header for Y4M and from the first image for MJPEG
 * (every later image must keep its size and sampling: a change is a reader
 * error that names the frame index); nbuf in [2, 64] slots; loop != 0
 * rewinds at end of file.  *handle owns a reader thread. */
int rv_capture_open(const char* path, int fmt, int W, int H, int nbuf, int loop, void** handle);
/* info[6] = {W, H, fmt, frame bytes (NV12: 3WH/2, BGR: 3WH, MJPEG: the
 * coefficient record's size), pinned, nbuf} */
int rv_capture_info(void* handle, int* info);
/* MJPEG sources: info[14] = {sampling code, components, then the twelve
 * values of rv_jpeg_record_layout for the source's records}. */
int rv_capture_jpeg_info(void* handle, int64_t* info);
/* Next frame in order (blocks until read): RV_OK with the slot's host pointer,
 * read time (s since the epoch) and frame index, or RV_EOF.  The slot stays
 * held until rv_capture_release. */
int rv_capture_next(void* handle, uint8_t** frame, double* ts, int64_t* index, int* slot);
int rv_capture_release(void* handle, int slot);
/* One frame of each of S sources -> dev + s * dev_stride (H2D on `stream`);
 * each slot returns to its reader once an event recorded behind its copy has
 * completed, so the rings refill while the device works.  ts / index (host, S) may be
 * NULL.  RV_EOF when a source ended (frames already queued are still
 * copied); rv_capture_close waits for copies still in flight. */
int rv_capture_upload_batch(void* const* handles, int S, uint8_t* dev, size_t dev_stride,
                            double* ts, int64_t* index, void* stream);
int rv_capture_close(void* handle);

/* ------------------------------------------------------------------------ */
/* Baseline JPEG (what cv2.imdecode / VideoCapture do for JPEG and MJPG with */
/* a default libjpeg build: "islow" IDCT, "fancy" chroma upsampling, 16-bit  */
/* fixed-point YCbCr -> RGB; uint8 output bit for bit).  The host parses the  */
/* markers and decodes the Huffman stream (csrc/jpeg_host.h), the device      */
/* does the rest (csrc/jpeg.hip).  Supported: SOF0, 8-bit, one interleaved    */
/* scan; three components with Y 1x1 / 2x1 / 2x2 and Cb, Cr 1x1 (4:4:4,        */
/* 4:2:2, 4:2:0) or one component (grey, B = G = R); DRI / RSTn; the Annex K  */
/* Huffman tables when an image has no DHT; APPn / COM skipped.  Progressive, */
/* extended, lossless, arithmetic, 12-bit, 16-bit quant tables, 4 components, */
/* other sampling factors and multi-scan files are RV_EINVAL with the cause   */
/* in rv_last_error.                                                          */
/*                                                                            */
/* Between the two halves travels a fixed-size coefficient record:            */
/*   int32[8]          {RV_JPEG_MAGIC, W, H, sampling code, components, 0..}  */
/*   uint16[ncomp][64] quant tables, natural order (index 8 v + u)            */
/*   per component     the MCU-padded block grid, row-major, each block 64    */
/*                     int16 quantised coefficients in natural order          */
/* rv_jpeg_record_layout gives the offsets: layout[12] = {record bytes,       */
/* components, quant offset, coefficient offset x 3, blocks across x 3,       */
/* blocks down x 3} (unused components 0).                                    */
/* ------------------------------------------------------------------------ */
#define RV_JPEG_MAGIC 0x46434a52
#define RV_JPEG_444 0
#define RV_JPEG_422 1
#define RV_JPEG_420 2
#define RV_JPEG_GRAY 3
/* Host only (no device needed).  info[4] = {W, H, sampling code, components}
 * of the image that starts at data[0]. */
int rv_jpeg_probe(const uint8_t* data, size_t n, int* info);
size_t rv_jpeg_record_bytes(int W, int H, int sampling); /* 0 for a bad size / code */
int rv_jpeg_record_layout(int W, int H, int sampling, int64_t* layout);
/* Entropy-decode one image into a record of at most `cap` bytes (host). */
int rv_jpeg_decode_coef(const uint8_t* data, size_t n, uint8_t* record, size_t cap);
/* S records of W x H images (device, record_stride bytes apart, 16-byte
 * aligned; their sampling may differ) -> (S, H, W, 3) BGR u8.  One kernel on
 * `stream`, no host reads.  W and H size the launch; a record whose header
 * does not say W x H, or that does not fit its stride, leaves its frame
 * unwritten. */
int rv_jpeg_coef_to_bgr_u8(const uint8_t* records, size_t record_stride, int S, int W, int H,
                           uint8_t* bgr, void* stream);

/* --- The way back: a baseline JPEG encoder whose output equals, byte for
 * byte, what libjpeg writes with its default settings and one restart
 * segment per MCU row (Pillow: save(quality=q, subsampling=s,
 * restart_marker_rows=1); cv2.imwrite's arithmetic).  16-bit fixed-point
 * RGB -> YCbCr, right edge replicated, h2v1 / h2v2 box downsampling with
 * libjpeg's alternating bias, the bottom edge padded per row group and then
 * per downsampled plane, "islow" forward DCT, quant tables of
 * jpeg_quality_scaling, the Annex K Huffman tables, JFIF 1.01 APP0.  Markers
 * in order: SOI, APP0, DQT, DQT, SOF0, DHT x 4, DRI, SOS, segments separated
 * by RSTm, EOI.  Colour input only: RV_JPEG_GRAY is RV_EINVAL in the device
 * entries.  The host half (csrc/jpeg_host.h) needs no device. */
/* Quant tables of `quality` (1..100), uint16[64] each, natural order. */
int rv_jpeg_quant_tables(int quality, uint16_t* luma, uint16_t* chroma);
/* SOI .. SOS of a W x H image (at most 640 bytes) -> out[0, *n); DRI only
 * when restart_interval_mcus > 0.  Sampling may be RV_JPEG_GRAY here. */
int rv_jpeg_write_header(int W, int H, int sampling, int quality, int restart_interval_mcus,
                         uint8_t* out, size_t cap, size_t* n);
/* Host: a coefficient record -> a complete image in out[0, *n), the inverse
 * of rv_jpeg_decode_coef for images that use the Annex K Huffman tables.
 * The quant tables come from the record; grey records are supported;
 * restart_interval_mcus = 0 writes no DRI.  RV_EINVAL when the image does
 * not fit `cap` or a value has no baseline code. */
int rv_jpeg_encode_coef(const uint8_t* record, size_t record_bytes, int restart_interval_mcus,
                        uint8_t* out, size_t cap, size_t* n);

/* A device stream is a 16-byte header, uint32[4] = {RV_JPEG_STREAM_MAGIC,
 * image bytes, flags, restart segments}, followed by the image.  "image
 * bytes" is the size the image needs, whether or not it fitted. */
#define RV_JPEG_STREAM_MAGIC 0x534a5652 /* "RVJS" */
#define RV_JPEG_STREAM_HEADER_BYTES 16
#define RV_JPEG_STREAM_OVERFLOW 1   /* header + image > capacity: image cut at capacity */
#define RV_JPEG_STREAM_BAD_RECORD 2 /* the record is not a W x H record of this sampling */
/* Worst-case stream size (header included, rounded up to 16), 0 for a bad
 * size or code: 16 + 640 (file header) + blocks x 416 + MCU rows x 4 + 2.  A
 * block takes at most 1660 bits = 208 bytes (DC: 11-bit code + 11 value bits;
 * 63 AC coefficients x (16-bit code + 10 value bits)), every byte of which
 * may be 0xFF and stuffed; a segment adds its padded last byte, stuffed, and
 * its RSTm. */
size_t rv_jpeg_stream_bound(int W, int H, int sampling);
/* (S, H, W, 3) BGR u8 frames (device, contiguous) -> S coefficient records in
 * the layout above (three components, quant tables of `quality`),
 * record_stride bytes apart, 16-byte aligned.  rv_jpeg_coef_to_bgr_u8 and the
 * host entries read them unchanged.  One kernel on `stream`, no host reads. */
int rv_jpeg_bgr_to_coef_u8(const uint8_t* bgr, int S, int H, int W, int sampling, int quality,
                           uint8_t* records, size_t record_stride, void* stream);
size_t rv_jpeg_stream_ws_bytes(int S, int W, int H, int sampling);
/* S device records of W x H colour images with this sampling -> S streams,
 * stream_stride bytes apart (4-byte aligned).  `header` (host, copied during
 * the call) is the SOI .. SOS prefix every image starts with, from
 * rv_jpeg_write_header with restart_interval_mcus = MCUs per MCU row; its
 * quant tables must be the records'.  Every MCU row is entropy-coded as its
 * own restart segment and the segments are compacted on the device.  No more
 * than `capacity` (<= stream_stride) bytes of a stream are written: a frame
 * that does not fit gets RV_JPEG_STREAM_OVERFLOW and the bytes that do fit.
 * `ws` (device, 16-byte aligned, rv_jpeg_stream_ws_bytes) is scratch.  Two
 * kernels on `stream`, no host reads. */
int rv_jpeg_coef_to_stream(const uint8_t* records, size_t record_stride, int S, int W, int H,
                           int sampling, const uint8_t* header, size_t header_bytes, uint8_t* ws,
                           size_t ws_bytes, uint8_t* streams, size_t stream_stride,
                           size_t capacity, void* stream);
size_t rv_jpeg_encode_ws_bytes(int S, int W, int H, int sampling);
/* Frames -> streams: the two entries above over `ws` (rv_jpeg_encode_ws_bytes:
 * the records and the entropy scratch). */
int rv_jpeg_encode_bgr_u8(const uint8_t* bgr, int S, int H, int W, int sampling, int quality,
                          uint8_t* ws, size_t ws_bytes, uint8_t* streams, size_t stream_stride,
                          size_t capacity, void* stream);

/* --- Motion-JPEG file sink (csrc/sink.hip; the reference's writer.write,
 * main_preview.py:130,137), the counterpart of rv_capture_*: one writer
 * thread per file over a ring of nbuf (2..64) pinned slots of `capacity`
 * bytes, the capacity the streams were encoded with.  The file holds the
 * images back to back, which RV_CAP_MJPEG reads; there is no MP4 / AVI muxer,
 * and no timing is stored. */
int rv_sink_open(const char* path, int nbuf, size_t capacity, void** handle);
/* Stream s of `streams` (device, rv_jpeg_encode_bgr_u8's output, stream_stride
 * >= capacity bytes apart) is appended to file handles[s].  The call records
 * an event on `stream` and returns; it never makes `stream` wait.  The writer
 * waits for the event, copies the stream header and then the image's bytes
 * rounded up to 4 KiB on a stream of its own, and writes the image.  Frames
 * reach the file in submission order.  A full ring blocks the caller.  The
 * device memory of a batch must stay unchanged until nbuf later calls have
 * returned (nbuf + 1 buffers in rotation do).  A frame that overflowed, a
 * stream without the magic and an I/O error are counted, nothing is written
 * for that frame, and the next call (and rv_sink_flush / rv_sink_close)
 * returns RV_EINVAL with the file and frame in rv_last_error. */
int rv_sink_write_batch(void* const* handles, int S, const uint8_t* streams, size_t stream_stride,
                        void* stream);
/* stats[8] = {frames submitted, frames written, bytes written, bytes copied
 * from the device, frames overflowed, other failed frames, nbuf, capacity} */
int rv_sink_stats(void* handle, int64_t* stats);
/* Wait until every submitted frame is in the file and flush it. */
int rv_sink_flush(void* handle);
/* Write what is queued, flush, close the file, free the ring. */
int rv_sink_close(void* handle);

/* --- Detection overlays and the compare canvas (csrc/overlay.hip; the
 * reference's draw_detections, src/vis/draw.py:25-102, and make_canvas,
 * main_preview.py:12-34).  What the reference computes itself is reproduced
 * exactly: which detections are drawn and in which order, the colours, the
 * label strings and every coordinate formula.  Its two OpenCV primitives
 * (cv2.rectangle, cv2.putText with Hershey strokes) are replaced by the
 * raster model below, with a fixed bitmap font; pixel parity with cv2's
 * antialiased text and round-joined thick outlines is not promised.
 *
 * Raster model.  Coordinates are integers and ranges inclusive.  Everything
 * is clipped to the image; colours are BGR u8, written opaque.
 *   - Painter's order: primitives apply in list order, the last one covering
 *     a pixel wins.  Per detection: box outline, top label box, top text, then
 *     bottom label box and bottom text when there are metrics.
 *   - RV_OVERLAY_FILL (x0,y0)-(x1,y1): every pixel with min(x0,x1) <= x <=
 *     max(x0,x1), the same in y (cv2's thickness -1).
 *   - RV_OVERLAY_OUTLINE, thickness t >= 1, a = t / 2, b = (t - 1) / 2: each
 *     edge line at coordinate c covers c-a .. c+b across and runs from outer
 *     corner to outer corner (square joins): the filled rectangle
 *     (x0-a, y0-a)-(x1+b, y1+b) minus the filled rectangle
 *     (x0+b+1, y0+b+1)-(x1-a-1, y1-a-1).  t = 1 is exactly cv2's pixels.
 *   - Font: csrc/overlay_font.h, 95 glyphs for ASCII 32..126, each a 6 x 11
 *     one-bit cell; rows 0..8 above the baseline, rows 9..10 descenders.  A
 *     byte outside 32..126 is drawn as '?'.
 *   - RV_OVERLAY_TEXT at origin (x0, y0) = (ox, oy), glyph scale k (1..8):
 *     byte i occupies x in [ox + 6k*i, ox + 6k*(i+1) - 1], cell row r occupies
 *     y in [oy - 9k + 1 + k*r, oy - 9k + k*(r+1)] (the last row above the
 *     baseline ends at y = oy); a set bit paints a k x k block.
 *   - Text metrics (for cv2.getTextSize): width 6k*len, height 9k, baseline
 *     2k, whatever the thickness.
 *   - Text thickness t (1..32; larger values draw as 32): 1 draws the glyphs
 *     as they are, t >= 2 the union of the glyphs shifted by every dx, dy in
 *     [-((t-1)/2), t/2] (a square dilation).
 *   - font_scale -> k on the host: k = max(1, min(8, int(font_scale * 22 / 7
 *     + 0.5))).
 *
 * Display list: a 16-byte header, int32[4] = {count, 0, 0, 0}, followed by
 * `count` records of RV_OVERLAY_PRIM_BYTES; unused bytes of a record are 0.
 * Stream s's list of a workspace starts at s * (16 + (5*dmax + 8) * 96). */
#define RV_OVERLAY_FILL 1
#define RV_OVERLAY_OUTLINE 2
#define RV_OVERLAY_TEXT 3
#define RV_OVERLAY_TEXT_BYTES 64
#define RV_OVERLAY_PRIM_BYTES 96
#define RV_OVERLAY_LIST_HEADER_BYTES 16
#define RV_OVERLAY_CANVAS_PRIMS 8 /* capacity of the canvas list (three label pairs) */
#define RV_OVERLAY_NAME_BYTES 32  /* a class name: at most 31 bytes and a NUL */
#define RV_OVERLAY_ANNOTATE 0
#define RV_OVERLAY_COMPARE_H 1
#define RV_OVERLAY_COMPARE_V 2
typedef struct rv_overlay_prim {
  int32_t kind;          /* RV_OVERLAY_FILL / OUTLINE / TEXT; anything else draws nothing */
  int32_t x0, y0;        /* a corner; text: the origin (left end of the baseline row) */
  int32_t x1, y1;        /* the opposite corner; text: 0 */
  uint8_t b, g, r;       /* colour */
  uint8_t thickness;     /* outline and text; fill: 0 */
  uint8_t scale;         /* text: k, 1..8; else 0 */
  uint8_t len;           /* text: bytes used of `text`, 0..64; else 0 */
  uint8_t pad[2];
  uint8_t text[RV_OVERLAY_TEXT_BYTES];
  int32_t reserved;
} rv_overlay_prim;
/* Bytes of S display lists of 5*dmax + 8 records each; 0 for a bad size. */
size_t rv_overlay_ws_bytes(int S, int dmax);
/* One step's device results -> S display lists, as draw_detections builds
 * them (draw.py:34-56 and its two label helpers) on H x W frames: slot i <
 * det_n[s] of dets (S, dmax, 6: x1 y1 x2 y2 conf cls) is drawn when, after
 * int() truncation, x2 > x1 and y2 > y1; a skipped detection leaves no gap.
 * Colour _COLOR_TABLE[cls % 10]; box thickness max(1, thickness), text
 * thickness one less (at least 1); glyph scale `scale`.  Top label
 * "ID <track_id> | <name> <conf:.2f>" (no prefix for track_id < 0; <name> is
 * names[cls] -- nc x 32 bytes, NUL-terminated -- or str(cls) when that is
 * empty or cls is outside [0, nc)); bottom label "<d:.1f> m / <v:.1f> km/h"
 * from distance_m / speed_kmh, where NaN means None (left out; both NaN: no
 * bottom label).  The numbers are formatted as Python's f-strings do,
 * correctly rounded half to even, for |x| < 1e9; anything larger prints
 * "---".  One kernel on `stream`, no host reads. */
int rv_overlay_layout(const float* dets, const int* det_n, const int* track_id,
                      const double* distance_m, const double* speed_kmh, int S, int dmax, int H,
                      int W, const uint8_t* names, int nc, int thickness, int scale,
                      uint8_t* lists, size_t lists_bytes, void* stream);
/* out[s] = the base image, then stream s's display list, then the canvas list.
 * RV_OVERLAY_ANNOTATE: the base is proc[s] (S, H, W, 3); `raw` is ignored and
 * out is (S, H, W, 3).  RV_OVERLAY_COMPARE_H / _V: the base is raw[s], a
 * divider of divider_px >= 0 pixels of colour (40, 40, 40), then proc[s], side
 * by side -- out (S, H, 2W + d, 3) -- or stacked -- out (S, 2H + d, W, 3); the
 * streams' lists are drawn at the PROC pane's offset and clipped to that
 * pane.  `lists` (device, may be NULL: nothing per stream) holds S lists for
 * `dmax`; counts are read on the device and capped at the capacity.
 * `canvas_list` (device, may be NULL) is one list of at most
 * RV_OVERLAY_CANVAS_PRIMS records in output coordinates, drawn on top of
 * every stream's image (the RAW / PROC / FPS labels).  proc and raw are only
 * read; `out` overlapping either is RV_EINVAL.  One kernel on `stream`: one
 * read and one write of every pixel, no host reads. */
int rv_overlay_raster(const uint8_t* proc, const uint8_t* raw, int S, int H, int W, int mode,
                      int divider_px, const uint8_t* lists, int dmax, const uint8_t* canvas_list,
                      uint8_t* out, void* stream);

/* --- Native launch schedule (csrc/sched.hip; no reference counterpart: the
 * reference runs its chain synchronously, main_preview.py:94-109).  A run of
 * K pipelined steps recorded once as a list of stream-ordered calls of this
 * library plus event record / wait nodes, issued by rv_sched_run with one
 * call.  rvs_amd/schedule.py records it.  Op argument arrays follow the C
 * signature of the op with float-class arguments moved, in order, to fargs
 * and the stream removed (it is the node's `stream`); a host-array argument
 * is passed as its byte offset into `host` (copied at record time) or -1. */
#define RV_SCHED_CLAHE_MEDIAN_LETTERBOX 0 /* rv_clahe_median_letterbox_u8 */
#define RV_SCHED_CLAHE_MEDIAN 1           /* rv_clahe_median_u8 */
#define RV_SCHED_LETTERBOX 2              /* rv_letterbox_u8 */
#define RV_SCHED_YOLO_FORWARD_PART 3      /* rv_yolo_forward_part */
#define RV_SCHED_NMS 4                    /* rv_nms_postprocess */
#define RV_SCHED_SORT_UPDATE 5            /* rv_sort_update */
#define RV_SCHED_HANDBACK 6               /* rv_results_handback */
#define RV_SCHED_UNTRACKED 7              /* rv_untracked_metrics */
#define RV_SCHED_PREPROCESS_CHAIN 8        /* rv_preprocess_chain_u8 */
#define RV_SCHED_SORT_UPDATE_CAMS 9 /* rv_sort_update_cams */
#define RV_SCHED_UNTRACKED_CAMS 10 /* rv_untracked_metrics_cams */
#define RV_SCHED_NUM_OPS 11
int rv_sched_create(void** handle);
int rv_sched_destroy(void* handle);
int rv_sched_add_op(void* handle, int op, const int64_t* iargs, int ni, const double* fargs,
                    int nf, const void* host, size_t host_bytes, void* stream);
/* An event recorded on `stream` at this point of the run; its id -> *event.
 * timing != 0: a timing event (rv_sched_event_elapsed). */
int rv_sched_add_record(void* handle, void* stream, int timing, int* event);
/* `stream` waits for event `event` (an earlier record node). */
int rv_sched_add_wait(void* handle, void* stream, int event);
int rv_sched_num_nodes(void* handle);
/* Host wait (this thread only) for record node `event` of the last run.
 * Valid only after rv_sched_run returned RV_OK for that run: RV_EINVAL
 * before the first run, while a run is issuing, after a run that failed
 * part-way, or for an event the latest run did not issue.  Single issuer:
 * waits must not overlap an rv_sched_run of the same handle from another
 * thread (issue a run, wait on its events, then issue the next run); the
 * RV_EINVAL check covers a wait that starts while a run is issuing, not a
 * run that starts while a wait polls. */
int rv_sched_event_sync(void* handle, int event);
/* Non-blocking form: 1 = completed, 0 = not yet, < 0 = error (same
 * validity rule as rv_sched_event_sync). */
int rv_sched_event_query(void* handle, int event);
/* Milliseconds between two timing record nodes of the last run (same
 * validity rule as rv_sched_event_sync). */
int rv_sched_event_elapsed(void* handle, int a, int b, float* ms);
/* Issue the whole schedule: every stream it uses waits for `origin`'s work
 * so far, the nodes are issued in record order, and `origin` waits for every
 * stream at the end.  Asynchronous (no host synchronisation). */
int rv_sched_run(void* handle, void* origin);

#ifdef __cplusplus
}
#endif
#endif /* RVHIP_H */
