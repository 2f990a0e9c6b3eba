/*
 * evam_pp.h — C ABI of the MI355X-native frame pre-processing backend.
 *
 * This is the drop-in boundary for the EVAM pre-process hot path:
 *   decoded NV12 / I420 / BGRx / BGR frame (device memory)
 *     -> optional ROI crop (gvaclassify)
 *     -> BT.601 colour conversion to BGR      (OpenCV cvtColor YUV2BGR_NV12 / _I420, BGRA2BGR)
 *     -> INTER_LINEAR resize                  (OpenCV resize, 8U fixed-point path)
 *     -> aspect-ratio letterbox / central crop (DL Streamer model-proc "resize"/"crop")
 *     -> optional BGR->RGB                    (model-proc "color_space")
 *     -> optional range + mean/std to fp32    (model-proc "range"/"mean"/"std")
 *        or, opt-in, to fp16 / bf16: that fp32 value rounded once, to nearest even, for a model bound in FP16
 *        (models_list/models.list.yml lists every model in FP16 and FP32). Planar 16-bit output runs on the same
 *        kernel families as fp32; interleaved (NHWC) 16-bit output is served by the generic kernel only (three
 *        element stores per pixel) — fast interleaved 16-bit variants are not built.
 *     -> planar NCHW write into batch slot n  (DL Streamer MatToMultiPlaneImage), or, with
 *        evam_tensor.layout = EVAM_LAYOUT_NHWC, the interleaved H x W x 3 image of that slot
 *        (Convert(..., make_planar = false): channels-last model input, published BGR frames)
 *
 * Reference interface replaced (all paths relative to the reference tree):
 *   - element selection surface: pipelines/object_detection/vehicle/pipeline.json:5,13-18
 *     ("detection-properties" element-properties passthrough), pipelines/object_classification/
 *     vehicle_attributes/pipeline.json:4-5,12-23, pipelines/action_recognition/general/pipeline.json:3-4,24-29;
 *     the parameters arrive through evas/manager.py:127-141 (pipeline.start(..., parameters=)).
 *   - native boundary [third party, not vendored]: DL Streamer 2022.1
 *     ImagePreprocessor::Convert(const Image& src, Image& dst, pre_proc_info, transform, make_planar,
 *     allocate_destination) selected by the element property "pre-process-backend" (SURVEY.md §8b).
 *     evam_pp_run() is that call batched over frames/ROIs; evam_image mirrors DLS `Image`,
 *     evam_preproc mirrors `InputImageLayerDesc`, evam_transform mirrors `ImageTransformationParams`.
 *
 * Conventions: every function returns EVAM_PP_OK (0) or a negative evam_pp_status; no C++ exception
 * crosses the ABI; the message of the last failure on the calling thread is evam_pp_last_error().
 * The caller owns every device buffer. A handle is bound to one HIP device and one HIP stream, is not
 * thread-safe, and launches asynchronously on that stream (evam_pp_sync() waits for it).
 */
#ifndef EVAM_PP_H
#define EVAM_PP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVAM_PP_ABI_VERSION 3 /* 2: evam_pp_run_slots; 3: evam_tensor.layout (sizeof 32 -> 40) */

/* DL Streamer FourCC values: fourcc(a,b,c,d) = a | b<<8 | c<<16 | d<<24. */
enum evam_fourcc {
    EVAM_FOURCC_NV12 = 0x3231564E, /* Y plane + interleaved UV plane (4:2:0), VA-API decode output   */
    EVAM_FOURCC_I420 = 0x30323449, /* Y, U, V planes (4:2:0), avdec_h264 output                       */
    EVAM_FOURCC_BGRX = 0x58524742, /* packed 4-byte BGRx (videoconvert, action_recognition template)  */
    EVAM_FOURCC_BGRA = 0x41524742, /* packed 4-byte BGRA, treated as BGRx                             */
    EVAM_FOURCC_BGR  = 0x20524742  /* packed 3-byte BGR                                               */
};

enum evam_pp_status {
    EVAM_PP_OK = 0,
    EVAM_PP_ERR_INVALID_ARG = -1, /* null pointer, bad size, bad enum, index out of range       */
    EVAM_PP_ERR_UNSUPPORTED = -2, /* fourcc / channel count / dtype not supported               */
    EVAM_PP_ERR_ALIGNMENT   = -3, /* plane pointer or pitch not a multiple of 16 bytes          */
    EVAM_PP_ERR_EMPTY_ROI   = -4, /* ROI is empty after clipping to the frame                   */
    EVAM_PP_ERR_HIP         = -5, /* a HIP runtime call failed (message has the HIP error)      */
    EVAM_PP_ERR_NO_DEVICE   = -6, /* no HIP device / bad device ordinal                         */
    EVAM_PP_ERR_OOM         = -7  /* device or host allocation failed                           */
};

/* A decoded frame. Planes are DEVICE pointers; plane i has pitch[i] bytes per row.
 * NV12: planes[0]=Y, planes[1]=UV.  I420: Y, U, V.  BGRx/BGRA/BGR: planes[0] only.
 * YUV 4:2:0 frames must have even width and height (as OpenCV's YUV420 conversions require).
 * Every used plane pointer and pitch must be a multiple of 16 bytes; nothing more is assumed about them. Every plane
 * has its own pitch, at least its row bytes (NV12's UV pitch need not equal its Y pitch, I420's U and V pitches need
 * not be equal nor half the Y pitch), and the frames of one call need not share pitches. The planes of a frame may lie
 * in any order and at any distance in memory (chroma below luma, V below U, separate allocations), and a frame may be
 * a window of a larger surface: plane pointers into its interior, the surface's pitch as the pitch. The only limits
 * are that a plane's pitch x rows stays under 2 GiB, and that I420 planes more than 2 GiB apart take a slower path.
 * Only the row bytes of every row are used as pixels, but the kernels fetch whole 16-byte chunks: every row must be
 * readable up to its row bytes rounded up to 16 (which its pitch covers). What lies in the padding, between the
 * planes or around a window never reaches the output. */
typedef struct evam_image {
    int32_t fourcc;
    int32_t width;
    int32_t height;
    int32_t pitch[3];
    const uint8_t* planes[3];
} evam_image;

/* One unit of work: a region of srcs[src_index]. w<=0 or h<=0 means the full frame.
 * ROIs are clipped to the frame; for 4:2:0 sources the clipped rect is then widened to even
 * coordinates: x0 = x & ~1, y0 = y & ~1, x1 = min(W, (x+w+1) & ~1), y1 = min(H, (y+h+1) & ~1). */
typedef struct evam_roi {
    int32_t src_index;
    int32_t x, y, w, h;
} evam_roi;

enum evam_resize_mode {
    EVAM_RESIZE_NO_ASPECT   = 0, /* plain resize to the tensor H x W (model-proc default)          */
    EVAM_RESIZE_ASPECT      = 1, /* model-proc resize=aspect-ratio: scale = min ratio, pad (letterbox) */
    EVAM_RESIZE_ASPECT_CROP = 2  /* resize=aspect-ratio + crop=central: scale = max ratio, centre crop */
};

enum evam_placement {
    EVAM_PLACE_TOP_LEFT = 0, /* letterbox image at (0,0), fill right/bottom (build default) */
    EVAM_PLACE_CENTER   = 1  /* letterbox image centred                                     */
};

enum evam_color_order { EVAM_COLOR_BGR = 0, EVAM_COLOR_RGB = 1 };
/* F16 / BF16: the fp32 value the F32 path stores, rounded once to the 16-bit type (round to nearest even; fp16 with
 * subnormals and overflow to +-inf; NaN stays NaN, the sign of zero is kept). Everything that holds for F32 holds for
 * them (norm_flags, range, mean, std, fill through the table, std[c] == 0 rejected); the element size is 2. A library
 * built before they existed answers them with EVAM_PP_ERR_UNSUPPORTED (the ABI version is unchanged: no struct grew). */
enum evam_dtype { EVAM_DTYPE_U8 = 0, EVAM_DTYPE_F32 = 1, EVAM_DTYPE_F16 = 2, EVAM_DTYPE_BF16 = 3 };

#define EVAM_NORM_RANGE    1 /* f = (float)u8 * ((max-min)/255) + min      (OpenCV convertTo) */
#define EVAM_NORM_MEAN_STD 2 /* f = (f - mean[c]) / std[c]                 (cv::subtract/divide) */

typedef struct evam_preproc {
    int32_t resize_mode;   /* evam_resize_mode                                                  */
    int32_t placement;     /* evam_placement (letterbox only)                                   */
    int32_t color_order;   /* evam_color_order of the output planes                             */
    int32_t out_dtype;     /* evam_dtype of the output tensor                                   */
    int32_t norm_flags;    /* EVAM_NORM_* bits; ignored for U8 output (F32, F16 and BF16 apply them) */
    uint8_t fill[4];       /* u8 fill value of padded pixels, per OUTPUT channel, before normalisation */
    float range[2];        /* {min, max}                                                        */
    float mean[3];         /* per OUTPUT channel                                                */
    float std[3];          /* per OUTPUT channel                                                */
} evam_preproc;

/* Element order inside one output slot (DLS Convert's make_planar flag).
 * NCHW: three planes of h*w elements, element (c, y, x) at c*h*w + y*w + x.
 * NHWC: one interleaved image, element (y, x, c) at (y*w + x)*3 + c.
 * c runs over the OUTPUT channel order either way: B,G,R, or R,G,B for EVAM_COLOR_RGB. */
enum evam_layout { EVAM_LAYOUT_NCHW = 0, EVAM_LAYOUT_NHWC = 1 };

/* Dense device tensor of n slots of 3*h*w elements. Item i is written to slot  slot_offset + i * slot_stride.
 * (slot_stride = 16, slot_offset = t % 16 packs a [S,16,3,H,W] clip ring.)
 * layout: evam_layout; a zero-initialised struct is planar. Any other value is EVAM_PP_ERR_INVALID_ARG.
 * data needs the alignment of one element only (a u8 NHWC view may start at an odd address). With
 * EVAM_LAYOUT_NHWC a slot's bytes (3*h*w*element size) must stay below 2 GiB. reserved is ignored. */
typedef struct evam_tensor {
    void* data;
    int32_t n, c, h, w;
    int32_t slot_offset;
    int32_t slot_stride;
    int32_t layout;
    int32_t reserved;
} evam_tensor;

/* Per-item transform for post-processing (DLS ImageTransformationParams): a resized-image pixel
 * (u, v) = ((x - crop_x) * scale_x, (y - crop_y) * scale_y); tensor pixel = (u + pad_x, v + pad_y). */
typedef struct evam_transform {
    float scale_x, scale_y;
    int32_t crop_x, crop_y, crop_w, crop_h;
    int32_t pad_x, pad_y;
    int32_t resized_w, resized_h;
} evam_transform;

/* Host-side accounting of the last evam_pp_run (filled when EVAM_OPT_STATS is on). */
typedef struct evam_pp_stats {
    int64_t src_bytes;   /* algorithmic source bytes: distinct touched rows x crop-window row bytes */
    int64_t dst_bytes;   /* output bytes written, padding included                                 */
    int32_t n_items;
    int32_t n_launches;
    float last_kernel_ms;/* duration of the last run's kernel(s) from HIP events (EVAM_OPT_TIMING) */
    uint32_t kernels;    /* kernel families the last run launched: EVAM_KERNEL_* bits (always filled)      */
} evam_pp_stats;

/* evam_pp_stats.kernels bits (diagnostics: which kernel family served a call). */
enum evam_kernel_family {
    EVAM_KERNEL_GENERIC = 1, EVAM_KERNEL_ROWS = 2, EVAM_KERNEL_STAGED = 4, EVAM_KERNEL_WAVE = 8,
    EVAM_KERNEL_STRIP = 16, EVAM_KERNEL_BAND = 32, EVAM_KERNEL_ROI = 64,
    EVAM_KERNEL_JPEG = 128, /* evam_pp_encode_jpeg: set beside the bits of the export that staged the BGR frame */
    EVAM_KERNEL_JPEG_DEC = 256, /* evam_pp_decode_jpeg: the only bit after a decode call */
    EVAM_KERNEL_DETOUT = 512 /* evam_pp_detection_output: the only bit after such a call */
};

enum evam_pp_option {
    EVAM_OPT_STATS  = 1, /* compute evam_pp_stats byte accounting on every run           */
    EVAM_OPT_TIMING = 2  /* bracket each run's kernels with HIP events on the handle's stream */
};

typedef struct evam_pp evam_pp;

/* Bind a handle to HIP device `hip_device` and stream `hip_stream` (NULL = the null stream). */
int evam_pp_create(int hip_device, void* hip_stream, evam_pp** out);

/* Pre-process n_items items (items == NULL: one full-frame item per src, n_items = n_srcs)
 * into dst. out_xform: NULL or an array of n_items. Asynchronous on the handle's stream. */
int evam_pp_run(evam_pp* h, const evam_image* srcs, int n_srcs, const evam_roi* items, int n_items,
                const evam_preproc* cfg, const evam_tensor* dst, evam_transform* out_xform);

/* evam_pp_run with an explicit output slot per item: item i is written to slot slots[i] of dst (dst->slot_offset
 * and dst->slot_stride are ignored). slots is a HOST array of n_items distinct values in [0, dst->n); a value
 * outside it or a slot given twice is EVAM_PP_ERR_INVALID_ARG. One launch can then write the new frames of many
 * camera streams into a shared [S,16,3,H,W] clip ring, each at its own stream's slot s*16 + t_s % 16, where the
 * reference's gvaactionrecognitionbin (pipelines/action_recognition/general/pipeline.json:3-4) pre-processes one
 * stream's frame per encoder call. */
int evam_pp_run_slots(evam_pp* h, const evam_image* srcs, int n_srcs, const evam_roi* items, int n_items,
                      const evam_preproc* cfg, const evam_tensor* dst, const int32_t* slots,
                      evam_transform* out_xform);

int evam_pp_sync(evam_pp* h);
int evam_pp_set_stream(evam_pp* h, void* hip_stream);
int evam_pp_set_option(evam_pp* h, int option, int value);
int evam_pp_get_stats(evam_pp* h, evam_pp_stats* out);
void evam_pp_destroy(evam_pp* h);
const char* evam_pp_last_error(void);
int evam_pp_abi_version(void);

/* Exact OpenCV INTER_LINEAR coefficient tables for a src_size -> dst_size axis, as the kernels compute
 * them on the device: ofs = clamped first tap (x axis) or raw floor (y axis), c0/c1 = 11-bit weights.
 * is_x != 0 applies OpenCV's x-axis border rule (fx = 0 at clamped taps). Host-only helper. */
int evam_pp_linear_table(int src_size, int dst_size, int is_x, int32_t* ofs, int16_t* c0, int16_t* c1);

/* The normalisation table the kernels map the resized u8 value through: 768 elements [c][u] (c = output channel,
 * u = 0..255) in cfg->out_dtype, written to out: 4 bytes each for EVAM_DTYPE_F32, 2 for F16 / BF16 (the fp32 entry
 * narrowed once, round to nearest even). evam_pp_run fills its device table from this same function. Only out_dtype,
 * norm_flags, range, mean and std are read. EVAM_DTYPE_U8 (no table) and std[c] == 0 with EVAM_NORM_MEAN_STD are
 * EVAM_PP_ERR_INVALID_ARG; an unknown dtype is EVAM_PP_ERR_UNSUPPORTED. Host-only helper. */
int evam_pp_norm_table(const evam_preproc* cfg, void* out);

/* ---- JPEG encoding of the published frame (the reference's publisher: cv2.imencode('.jpg', frame,
 * [IMWRITE_JPEG_QUALITY, level]), evas/publisher.py:127-151). Added without a struct change, so the ABI version
 * stays 3; a library built before them lacks the symbols.
 *
 * The file is what libjpeg writes with its defaults: baseline JFIF 1.01, 4:2:0, JDCT_ISLOW, the Annex K Huffman
 * tables, no restart interval, quantisation tables of jpeg_set_quality(quality, TRUE) (a quality <= 0 counts as 1).
 * The pixels are the frame evam_pp_run publishes as an identity BGR u8 export, converted by libjpeg's integer
 * RGB -> YCbCr. tests/jpeg_ref.py restates the arithmetic and is pinned byte for byte to libjpeg-turbo files. */

/* The 623 bytes every file of (width, height, quality) starts with: SOI, APP0, two DQT, SOF0, four DHT, SOS.
 * *len is set to 623 whenever len is given; out must hold that many (cap). Host-only helper. */
int evam_pp_jpeg_header(int width, int height, int quality, uint8_t* out, size_t cap, size_t* len);

/* Worst-case bytes of one encoded frame, header and EOI included: a block codes to at most 1,660 bits (DC 11 + 11,
 * AC 63 x (16 + 10)), doubled for byte stuffing, six blocks per 16x16 MCU. 0 for a size evam_pp_run refuses.
 * Host-only helper. */
size_t evam_pp_jpeg_bound(int width, int height);

/* Encode every frame of srcs (one size per call; any fourcc evam_pp_run accepts, full frame, source size) as one
 * JFIF file each. Frame i's file starts at dst + i*dst_stride (device memory). sizes[i] (device, uint32) is its full
 * length in bytes, also when that exceeds dst_stride: then nothing is written outside the slot, the slot's contents
 * are unspecified, and the caller retries with a larger stride (evam_pp_jpeg_bound always suffices).
 * quality: 0..100. EVAM_PP_ERR_INVALID_ARG: another quality, frames of different sizes, n_srcs outside 1..65535, a
 * null pointer, dst_stride smaller than the header plus 2, a frame of more than 2^32 / 1660 blocks. Sources are
 * validated as evam_pp_run validates them, with its status codes. Scratch belongs to the handle, grows on demand and
 * is reused (EVAM_PP_ERR_OOM when it cannot). Asynchronous on the handle's stream. */
int evam_pp_encode_jpeg(evam_pp* h, const evam_image* srcs, int n_srcs, int quality,
                        void* dst, size_t dst_stride, uint32_t* sizes);

/* ---- Device-resident detections (gvadetect -> gvaclassify with no host round trip). Added without a struct change,
 * so the ABI version stays 3; a library built before them lacks the symbols.
 *
 * The host path of a detect -> classify chain copies the detector's [N,K,7] output back, parses it, maps the boxes
 * through the item transforms, filters them and hands evam_pp_run an evam_roi array. The calls below keep those rects
 * on the device: evam_pp_ssd_rois writes them into a device list, evam_pp_run_device_rois crops them from it. */

/* A list of ROIs in DEVICE memory: rois has room for cap entries; *count is the number of entries the producer
 * accepted, which may exceed cap (then only the first cap are stored). Both pointers are the caller's. */
typedef struct evam_roi_list {
    evam_roi* rois;
    uint32_t* count;
    int32_t cap;
    int32_t reserved;
} evam_roi_list;

/* SSD DetectionOutput rows -> the rects a gvaclassify stage crops. det: device float[n_items][k][7], rows of
 * (image_id, label, conf, x0, y0, x1, y1), box normalised to the tensor_w x tensor_h model input. Item i belongs to
 * srcs[i] (HOST array; only width and height are read) and to xf[i] (HOST array of the transforms evam_pp_run returned
 * for the detector's input, or NULL when every item was a plain full-frame resize). Per item, only the rows before
 * the first image_id < 0 count. A row is accepted when conf >= threshold (compared as floats), its label truncated to
 * an integer is one of labels[0, n_labels) (HOST array; NULL: every label), and the rect
 *   x = floor(x0' * W + 0.5), w = floor((x1' - x0') * W + 0.5)   (y, h alike; x0', x1' the box mapped to the frame
 *   through the transform and clipped to [0, 1], all in double)
 * has w > 0, h > 0 and a non-empty intersection with the frame. A row with a non-finite box value is rejected.
 * Accepted rects are written as evam_roi {src_index = i, x, y, w, h} in item order, then row order (an ordered
 * compaction: the order of the host path); *list->count receives their total, list->rois the first list->cap.
 * n_items and k: 1 .. 65535 each is served (EVAM_PP_ERR_INVALID_ARG beyond, for a NULL pointer, cap <= 0,
 * n_labels < 0 or a tensor size <= 0). Asynchronous on the handle's stream; the host reads no device memory. */
int evam_pp_ssd_rois(evam_pp* h, const float* det, int n_items, int k, const evam_image* srcs,
                     const evam_transform* xf, int tensor_w, int tensor_h, float threshold,
                     const int32_t* labels, int n_labels, const evam_roi_list* list);

/* evam_pp_ssd_rois on HOST arrays (det, list->rois and list->count are host memory): the same shared arithmetic,
 * for tests and for callers that already hold the detections on the host. Host-only helper. */
int evam_pp_ssd_rois_host(const float* det, int n_items, int k, const evam_image* srcs,
                          const evam_transform* xf, int tensor_w, int tensor_h, float threshold,
                          const int32_t* labels, int n_labels, const evam_roi_list* list);

/* evam_pp_run with the items taken from a device list: entry i, for i < min(*list->count, list->cap), is cropped
 * from srcs[entry.src_index] and written to slot dst->slot_offset + i * dst->slot_stride. Slots from the count on are
 * not touched. dst must hold the slot of entry cap - 1.
 * status: NULL or a device int32[cap]. status[i] is 0, or EVAM_PP_ERR_EMPTY_ROI / EVAM_PP_ERR_INVALID_ARG for a rect
 * that clips to nothing / a src_index outside [0, n_srcs); the slot of such an entry is not touched and every other
 * entry is processed as usual. Entries from the count on have status 0.
 * The host never reads the list and the call does not synchronise; it uploads a per-source table (planes, pitches,
 * size) only. The launch covers cap entries in list order: a workgroup whose entry is past the count or invalid
 * returns at once, so size cap for the detections expected, not for the worst case.
 * Refused, with nothing launched: sources of more than one fourcc, EVAM_LAYOUT_NHWC, an output size the ROI kernel
 * does not plan (EVAM_PP_ERR_UNSUPPORTED each); cap <= 0 or a NULL list / rois / count pointer
 * (EVAM_PP_ERR_INVALID_ARG). Sources, cfg and dst are validated as evam_pp_run validates them.
 * evam_pp_stats.kernels reports EVAM_KERNEL_ROI; n_items is cap; src_bytes is 0 (the rects are unknown to the host). */
int evam_pp_run_device_rois(evam_pp* h, const evam_image* srcs, int n_srcs, const evam_roi_list* list,
                            const evam_preproc* cfg, const evam_tensor* dst, int32_t* status);

/* ---- JPEG decoding of source frames (the reference's `{auto_source} ! decodebin` on the cv2.imencode('.jpg') blobs
 * of its message bus, evas/subscriber.py:92-106, pipelines/object_detection/app_src_dst/pipeline.json:3). Added
 * without a struct change, so the ABI version stays 3; a library built before them lacks the symbols.
 *
 * The pixels are libjpeg's default decode (what cv2.imdecode and jpegdec run): JDCT_ISLOW, fancy up-sampling,
 * integer YCbCr -> RGB, byte for byte. Served: baseline sequential DCT (SOF0), 8-bit samples, one interleaved scan,
 * 1 component or 3 with luma sampling (1,1), (2,1) or (2,2) and chroma (1,1), 8-bit DQT, up to two DC and two AC
 * Huffman tables taken from the file, DRI / RSTn, APPn and COM skipped, JFIF and Adobe (transform 1) files, width and
 * height 1..32768, files below 2^28 bytes.
 * The header parse refuses with EVAM_PP_ERR_UNSUPPORTED (nothing launched): SOF1/2/3/5.. (extended, progressive,
 * lossless, arithmetic), 12-bit samples, 2 or 4 components, any other sampling, 16-bit DQT, more than one scan, a scan
 * with spectral selection other than 0..63 or a successive-approximation byte other than 0, Adobe transform != 1 with
 * 3 components. EVAM_PP_ERR_INVALID_ARG: no SOI, a segment length that runs past len, a scan that names a table the
 * file never defined, a zero size. */
typedef struct evam_jpeg_info {
    int32_t width, height;
    int32_t components;        /* 1 (grey) or 3 (YCbCr) */
    int32_t h_samp, v_samp;    /* luma sampling factors: (1,1), (2,1) or (2,2); chroma is (1,1) */
    int32_t restart_interval;  /* MCUs, 0 = none */
    uint32_t scan_offset;      /* first byte of entropy-coded data */
} evam_jpeg_info;

/* Parse the markers up to and including SOS. Host-only helper. */
int evam_pp_jpeg_info(const uint8_t* file, size_t len, evam_jpeg_info* out);

/* Decode n files of one geometry (HOST bytes; width, height, components, sampling and restart interval shared) into
 * out[i] (HOST descriptors, DEVICE planes, fourcc BGR or BGRX, one fourcc per call; BGRX writes X = 255). Row padding
 * beyond width x bytes per pixel is never written. status: device int32[n]; status[i] is 0, or EVAM_PP_ERR_INVALID_ARG
 * for a scan that is no valid baseline scan (a bit pattern that is no code of the active table, a DC category above
 * 11 or an AC size above 10, a run past coefficient 63, a DC sum that leaves int16, data that ends before the last
 * MCU, an RSTn out of sequence or missing). The pixels of such a file are unspecified, but every byte written for it
 * lies inside its own out[i] rows; for any byte sequence every loop of the decoder ends and every access is in bounds.
 * EVAM_PP_ERR_INVALID_ARG besides the parse's: files that differ in geometry, out[i] of another size, of a fourcc
 * other than BGR / BGRX, or with a plane pointer or pitch that is no multiple of 16, n outside 1..65535, a NULL
 * pointer, an out[i] whose pitch x height reaches 2 GiB (a limit of this build, below the 4 GiB of a 32768 x 32768
 * BGRX frame: larger outputs are untested and refused), files of one call that hold 4 GiB or more together.
 * The file bytes are copied into pinned staging of the handle before the call returns (the caller may free
 * them) and from there to device scratch, which grows on demand and is reused (EVAM_PP_ERR_OOM when it cannot).
 * Asynchronous on the handle's stream, with one limit: a handle owns ONE staging buffer, so a call first waits (on
 * the host) until the previous decode call's upload has left the staging. That upload is queued on the stream behind
 * the kernels of the call before it, so on a busy stream at most one decode call runs while the next is staged: the
 * host is not free to queue many calls ahead. Growing a scratch buffer also waits for the work that uses it.
 * Callers that must queue several decode calls without a host wait use one handle per call in flight.
 * evam_pp_stats.kernels reports EVAM_KERNEL_JPEG_DEC. */
int evam_pp_decode_jpeg(evam_pp* h, const uint8_t* const* files, const size_t* lens, int n,
                        const evam_image* out, int32_t* status);

/* evam_pp_decode_jpeg on HOST memory only (out planes and status are host pointers): the same shared arithmetic,
 * driven sequentially, for tests and for callers without a device. Host-only helper. */
int evam_pp_decode_jpeg_host(const uint8_t* const* files, const size_t* lens, int n,
                             const evam_image* out, int32_t* status);

/* ---- JPEG sources as raw 4:2:0 planes (what the reference's `decodebin` hands gvadetect: jpegdec's I420 planes, which
 * the pre-processor then converts with the limited-range BT.601 arithmetic of evam_pp_run). Symbols added, no struct
 * changed: the ABI version stays 3.
 *
 * evam_pp_decode_jpeg with out[i] of fourcc NV12 or I420 (one fourcc per call): the planes are what libjpeg's
 * jpeg_read_raw_data returns, every component's jpeg_idct_islow output after the range limit, with no up-sampling and
 * no colour conversion. Y is cropped to width x height; Cb is cropped to width/2 x height/2 and becomes U, Cr
 * likewise V; NV12 interleaves U, V. Each used plane of out[i] (NV12: 0, 1; I420: 0, 1, 2) has its own pointer and
 * pitch, both multiples of 16, the pitch at least the row bytes, pitch x rows below 2 GiB; planes may lie in any order
 * and at any distance and may be windows of a larger surface. Only pixel bytes are ever written: width bytes of each
 * of height luma rows, and width (NV12) or width/2 (I420) bytes of each of height/2 chroma rows. Row padding, the gap
 * between planes and the surface around a window are never touched, for a damaged file as well.
 * Served: 3-component files with luma sampling (2,2) and even width and height (what evam_image admits for 4:2:0).
 * Any other file is refused with EVAM_PP_ERR_UNSUPPORTED before any work ("sampling" / "odd" in the message, which
 * names files[i]); such a file still decodes to BGR / BGRX with evam_pp_decode_jpeg. Every other refusal, the status
 * array, restart intervals, damaged scans and the staging are those of evam_pp_decode_jpeg.
 * evam_pp_stats.kernels reports EVAM_KERNEL_JPEG_DEC; n_launches is 5 (no component planes in scratch and no colour
 * pass: the IDCT kernel writes the caller's planes). */
int evam_pp_decode_jpeg_planes(evam_pp* h, const uint8_t* const* files, const size_t* lens, int n,
                               const evam_image* out, int32_t* status);

/* evam_pp_decode_jpeg_planes on HOST memory only (host planes, host status). Host-only helper. */
int evam_pp_decode_jpeg_planes_host(const uint8_t* const* files, const size_t* lens, int n,
                                    const evam_image* out, int32_t* status);

/* ---- gvatrack: object ids for detections and the reclassify-interval gate (the reference's `gvadetect ! gvatrack !
 * gvaclassify` templates, pipelines/object_tracking/person_vehicle_bike and object_line_crossing, with the element
 * properties tracking-type and reclassify-interval). Symbols and new structs added, no existing struct changed: the ABI
 * version stays 3.
 *
 * DL Streamer's tracker is closed; the rule here is this project's own, in integer arithmetic only, so
 * the host and the device agree bit for bit. Per stream: next_id (from 1) and EVAM_TRACK_SLOTS track slots. One step
 * takes the stream's frame index and the frame's detections (label, x, y, w, h) in list order:
 *   1. only the first EVAM_TRACK_DETS detections take part; the rest get id 0;
 *   2. a live track and a detection of the same label score key = (inter << 16) / union (integer division; inter the
 *      area of the rect intersection, union = area_t + area_d - inter, a box side counted as min(max(side, 0), 2^20));
 *      the pair is a candidate when union > 0 and key >= floor(iou_threshold * 65536);
 *   3. until no candidate is left among unmatched tracks and detections, the one with the largest key is matched
 *      (ties: lower slot, then lower detection index);
 *   4. a match copies the detection's box into the track, sets lost = 0 and gives the detection the track's id;
 *   5. every unmatched live track gets lost += 1 and is freed when lost > max_lost;
 *   6. unmatched participating detections, in order, take the lowest free slot (slots freed in 5 included) with
 *      id = next_id++, lost = 0, classified_at = EVAM_TRACK_NONE; with no free slot the detection gets id 0;
 *   7. the gate, when a classify label set is given: a detection whose label is in the set is due when its id is 0, or
 *      its track's classified_at is EVAM_TRACK_NONE, or frame - classified_at >= reclassify; a due detection with an
 *      id sets classified_at = frame. (What the pipeline's gvaclassify stage does with its per-object cache.)
 * Frame indices of a stream ascend and stay below EVAM_TRACK_NONE. */
#define EVAM_TRACK_SLOTS 128
#define EVAM_TRACK_DETS 128
#define EVAM_TRACK_NONE 0xFFFFFFFFu

typedef struct evam_track_slot { /* 32 B */
    uint32_t id;            /* 0: the slot is free */
    int32_t label;
    int32_t x, y, w, h;     /* the box of the last match */
    int32_t lost;           /* frames since the last match */
    uint32_t classified_at; /* frame index of the last due detection, or EVAM_TRACK_NONE */
} evam_track_slot;

/* A stream's tracker state (4128 B). A fresh state is all zero except next_id = 1 and every classified_at =
 * EVAM_TRACK_NONE; evam_pp_track_host initialises a state whose next_id is 0 (zeroed memory) that way itself. */
typedef struct evam_track_state {
    uint32_t next_id;
    uint32_t reserved[7];
    evam_track_slot slots[EVAM_TRACK_SLOTS];
} evam_track_state;

/* max_lost: 0 (tracking-type zero-term-imageless) .. 8 (short-term-imageless) and beyond; < 0 is refused.
 * iou_threshold: 0.3 by default in the pipeline; a value <= 0 makes every same-label pair a candidate. */
typedef struct evam_track_cfg {
    int32_t max_lost;
    float iou_threshold;
} evam_track_cfg;

/* One item (frame) of a track call: the tracker's stream slot it belongs to and its stream's frame index. */
typedef struct evam_track_item {
    int32_t stream;
    uint32_t frame;
} evam_track_item;

/* One step of the rule on HOST arrays: dets[n_dets] (src_index is ignored) with labels[n_dets] against *state.
 * ids: uint32[n_dets]. due: NULL or uint8[n_dets], 1 for a due detection. The gate runs when classify_labels is given
 * (n_classify_labels >= 0 entries) or when n_classify_labels < 0 with a NULL pointer (every label); a NULL pointer with
 * n_classify_labels == 0 runs no gate (due is all 0). The gate runs with or without a due array: classified_at is set
 * for every due detection either way, as on the device. reclassify >= 1. n_dets >= 0 (NULL arrays allowed when 0).
 * Needs no GPU. Host-only helper. */
int evam_pp_track_host(evam_track_state* state, const evam_track_cfg* cfg, uint32_t frame, const evam_roi* dets,
                       const int32_t* labels, int n_dets, const int32_t* classify_labels, int n_classify_labels,
                       int reclassify, uint32_t* ids, uint8_t* due);

/* A tracker: the states of n_streams streams (1..65535) in DEVICE memory it owns, all fresh. It belongs to the
 * device of h; any handle of that device may drive it, and calls through different handles (different HIP streams) are
 * ordered one behind the other on the device by an event the tracker owns: each call waits for the one before it, in
 * the order the host issued them, and the host does not wait (but see the due-flag buffer of
 * evam_pp_track_device_rois). The calls of one tracker come from one host thread at a time. */
typedef struct evam_pp_tracker evam_pp_tracker;
int evam_pp_tracker_create(evam_pp* h, int n_streams, const evam_track_cfg* cfg, evam_pp_tracker** out);
/* Waits for the tracker's last call, then frees it. */
void evam_pp_tracker_destroy(evam_pp_tracker* t);
/* Make stream slot `stream` fresh again (its stream ended). Asynchronous on the handle's stream. */
int evam_pp_tracker_reset(evam_pp* h, evam_pp_tracker* t, int stream);
/* Copy stream slot `stream`'s state to HOST memory `out`, behind every call issued so far, and wait for it
 * (diagnostics and tests: the only call here that synchronises). */
int evam_pp_tracker_read(evam_pp* h, evam_pp_tracker* t, int stream, evam_track_state* out);

/* The rule over a device list. list: the detections of n_items items in item order (entry.src_index = item, ascending,
 * as evam_pp_ssd_rois writes it); labels: device int32[list->cap], the label of each entry. items: HOST table of
 * n_items entries; the items of a stream slot must be contiguous in it and in ascending frame order, else
 * EVAM_PP_ERR_INVALID_ARG (as for a stream slot outside the tracker). Each stream slot in the table takes one step per
 * item of its own, in table order; an item without entries is a step with no detections.
 * ids: device uint32[list->cap]; ids[e] receives the id of entry e for e < min(*list->count, list->cap); an entry
 * whose src_index is outside [0, n_items) and the entries from the count on get 0.
 * classify_labels (HOST array) / n_classify_labels / reclassify: the gate, as for evam_pp_track_host.
 * due: NULL, or a second list (other memory than `list`) that receives the due entries, unchanged, in list order: an
 * ordered compaction with no atomic append. *due->count is the true total even past due->cap (then the first due->cap
 * are stored); classified_at is set for every due entry, stored or not.
 * One 256-thread workgroup per stream slot in the table walks that slot's items in order, state and keys in LDS.
 * Asynchronous on the handle's stream; the host reads no device memory. n_items 1..65535.
 * One exception to "asynchronous": with a due list the tracker keeps a buffer of list->cap due flags. It grows to the
 * largest cap seen; growing frees the old buffer, and that free waits for the device's pending work. Callers that
 * must never wait pass lists of one capacity (or the largest first): the buffer is then allocated once per tracker. */
int evam_pp_track_device_rois(evam_pp* h, evam_pp_tracker* t, const evam_roi_list* list, const int32_t* labels,
                              int n_items, const evam_track_item* items, const int32_t* classify_labels,
                              int n_classify_labels, int reclassify, uint32_t* ids, const evam_roi_list* due);

/* evam_pp_ssd_rois that also writes each accepted row's label, int(label) as the host path truncates it (0 for a label
 * that is not finite or outside int32), to out_labels[position] (device int32[list->cap]) beside its rect.
 * out_labels == NULL is evam_pp_ssd_rois itself: the same kernels, the same bytes. */
int evam_pp_ssd_rois_ex(evam_pp* h, const float* det, int n_items, int k, const evam_image* srcs,
                        const evam_transform* xf, int tensor_w, int tensor_h, float threshold,
                        const int32_t* labels, int n_labels, const evam_roi_list* list, int32_t* out_labels);

/* ---- SSD DetectionOutput: raw detector heads -> the [N, K, 7] rows evam_pp_ssd_rois and the host parser read (the
 * last layer of the OpenVINO IR of every detector the reference lists, models_list/models.list.yml; a PyTorch port of
 * such a model ends at its box deltas and class probabilities). Symbols and one new struct added, no existing struct
 * changed: the ABI version stays 3.
 *
 * OpenVINO's layer is third party and not vendored; the rule below is this project's own and follows
 * the published DetectionOutput-1 semantics for code_type = CENTER_SIZE, share_location = true, normalized = true,
 * variance_encoded_in_target = false, no clipping, decrease_label_id = false. No byte parity with OpenVINO is claimed.
 *
 * Inputs, all float32: loc[N][P][4] box deltas; conf[N][P][C] probabilities, prior-major and class-minor, softmax
 * already applied; priors[2][P][4] shared by the batch, row 0 the prior boxes (xmin, ymin, xmax, ymax), row 1 the four
 * variances of each prior. Per image n, in float32 with no contraction:
 *   1. class c != background_label, prior p: s = conf[n][p][c] is a candidate when s is finite and
 *      s > confidence_threshold;
 *   2. within a class: score descending, ties to the lower p; only the first top_k take part;
 *   3. a participating candidate is decoded: pw = pxmax - pxmin, ph = pymax - pymin, pcx = (pxmin + pxmax) * 0.5f,
 *      pcy alike, cx = ((v0 * l0) * pw) + pcx, cy = ((v1 * l1) * ph) + pcy, w = evam_expf(v2 * l2) * pw,
 *      h = evam_expf(v3 * l3) * ph, box = (cx - w * 0.5f, cy - h * 0.5f, cx + w * 0.5f, cy + h * 0.5f). evam_expf is
 *      the library's own exp (evam_pp_expf): +, *, one round-to-nearest and an exponent insert, the same bits on the
 *      host and the device, at most 2 ulp from the correctly rounded value on [-20, 20]. A candidate whose box has a
 *      non-finite value is dropped: it does not take part and does not suppress;
 *   4. greedy NMS within the class, in the order of 2: a candidate is kept when jaccard(it, k) <= nms_threshold for
 *      every kept k before it. jaccard is 0 when the boxes are disjoint (b.xmin > a.xmax || b.xmax < a.xmin, likewise
 *      in y) or when iw <= 0 || ih <= 0; otherwise inter / ((area_a + area_b) - inter), one IEEE float division;
 *      area = 0 for xmax < xmin || ymax < ymin, otherwise (xmax - xmin) * (ymax - ymin);
 *   5. of all kept candidates of the image the keep_top_k with the highest score survive; ties go to the lower class,
 *      then the lower p;
 *   6. out[n][K][7], K = keep_top_k: the survivors ordered by class ascending, then score descending, then p
 *      ascending, one row (float(n), float(c), s, xmin, ymin, xmax, ymax) each; EVERY row from the survivor count on
 *      is (-1, 0, 0, 0, 0, 0, 0), so the whole block is defined. counts[n] is the survivor count.
 * Limits (EVAM_PP_ERR_INVALID_ARG outside them, the message names the argument): n 1..65535; p >= 1 and
 * p * num_classes < 2^31; num_classes 2..EVAM_DETOUT_MAX_CLASSES; background_label -1 (none) .. num_classes - 1;
 * top_k and keep_top_k 1..EVAM_DETOUT_MAX_TOP_K (OpenVINO's -1, "all", is refused); confidence_threshold finite and
 * >= 0; nms_threshold finite. Any other attribute set of the layer (CORNER code types, per-class locations, clipping,
 * ...) cannot be expressed in evam_detout_cfg; the Python binding refuses it with EVAM_PP_ERR_UNSUPPORTED. */
#define EVAM_DETOUT_MAX_TOP_K 1024
#define EVAM_DETOUT_MAX_CLASSES 256

typedef struct evam_detout_cfg { /* 24 B */
    int32_t num_classes;        /* C */
    int32_t background_label;   /* -1: none */
    int32_t top_k;
    int32_t keep_top_k;         /* K */
    float confidence_threshold;
    float nms_threshold;
} evam_detout_cfg;

/* loc, conf, priors, out (float[n][keep_top_k][7]) and counts (uint32[n], or NULL) are DEVICE pointers. Two launches:
 * one 256-thread workgroup per (image, class) selects, orders, decodes and suppresses; one per image merges and
 * writes. The result does not depend on scheduling (no float atomics, no order taken from an atomic counter).
 * Scratch (n * num_classes * top_k keys of 8 bytes) belongs to the handle, grows on demand and is reused
 * (EVAM_PP_ERR_OOM when it cannot; growing waits for the work that uses the old buffer). Asynchronous on the handle's
 * stream; the host reads no device memory. evam_pp_stats.kernels reports EVAM_KERNEL_DETOUT, n_launches 2. */
int evam_pp_detection_output(evam_pp* h, const float* loc, const float* conf, const float* priors, int n, int p,
                             const evam_detout_cfg* cfg, float* out, uint32_t* counts);

/* evam_pp_detection_output on HOST arrays: the same shared arithmetic, driven sequentially. Needs no GPU.
 * Host-only helper. */
int evam_pp_detection_output_host(const float* loc, const float* conf, const float* priors, int n, int p,
                                  const evam_detout_cfg* cfg, float* out, uint32_t* counts);

/* The exp of step 3, so that tests and callers can reach it. Host-only helper. */
float evam_pp_expf(float x);

#ifdef __cplusplus
}
#endif

#endif /* EVAM_PP_H */
