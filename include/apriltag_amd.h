/* apriltag_amd.h -- C ABI of the MI355X-native AprilTag detector (libapriltag_amd.so).
 *
 * Drop-in boundary for the detector calls the reference node makes into NVIDIA's closed
 * cuAprilTags library (paths relative to /root/reference/isaac_ros_apriltag/):
 *
 *   amdCreateAprilTagsDetector   replaces nvCreateAprilTagsDetector   src/apriltag_node.cpp:450-452
 *   amdAprilTagsDetect           replaces cuAprilTagsDetect           src/apriltag_node.cpp:491-493
 *   amdAprilTagsDestroy          replaces cuAprilTagsDestroy          src/apriltag_node.cpp:556
 *   amdAprilTagsImageInput_t     replaces cuAprilTagsImageInput_t     src/apriltag_node.cpp:481-486
 *   amdAprilTagsID_t             replaces cuAprilTagsID_t             src/apriltag_node.cpp:412-419,509-516
 *   amdAprilTagsCameraIntrinsics_t replaces cuAprilTagsCameraIntrinsics_t  src/apriltag_node.cpp:447
 *   amdAprilTagsFamily           replaces cuAprilTagsFamily           src/apriltag_node.cpp:401-407
 *
 * Differences that are part of the contract (north_star of BASELINE.json):
 *   - the image is mono8 (1 byte/pixel, pitch-linear, DEVICE memory) for the calls above; colour frames as the reference
 *     feeds them -- rgb8 / bgr8 `uchar3` on its cuAprilTags branch (src/apriltag_node.cpp:469-486), the encoding table of
 *     :76-82 on its VPI branch -- go through amdAprilTagsDetectColor / amdAprilTagsDetectBatchColor /
 *     amdAprilTagsSubmitBatchColor, whose threshold pass reads the interleaved frame itself (no separate conversion launch
 *     at tile_size 4, decimate 1); amdAprilTagsConvertToMono8 remains as the stand-alone conversion
 *     (vpiSubmitConvertImageFormat, src/apriltag_node.cpp:275-282);
 *   - a batched entry point (amdAprilTagsDetectBatch) processes independent frames in one
 *     submission -- also in two halves, amdAprilTagsSubmitBatch / amdAprilTagsWaitBatch, so that a host
 *     overlaps its next host-to-device copy with the detection; a HIP stream replaces the CUDA stream;
 *   - more than one tag family can be enabled (amdCreateAprilTagsDetectorEx); tile_size is the
 *     reference's parameter (src/apriltag_node.cpp:566, handed over at :451): 4 or 8;
 *   - the skew K[0][1] of the reference's VPI path (src/apriltag_node.cpp:215-225) is a field of the
 *     configuration and, per frame of a batch, amdAprilTagsSetFrameSkews.
 * Ownership and threading follow the reference's use: the caller owns the input buffers and the
 * output arrays (host memory); the library owns everything behind the handle; one thread per handle;
 * every Detect call is host-synchronous (results valid on return).  All functions return 0 on
 * success and a non-zero amdAprilTagsStatus otherwise (the node drops the frame on a non-zero
 * detect status and throws on a non-zero create status, src/apriltag_node.cpp:453-457,494-497).
 *
 * Plain C, no C++ or torch types.  hipStream_t is passed as void* so that this header needs no HIP
 * include; pass NULL for the detector's own stream.
 */
#ifndef APRILTAG_AMD_H_
#define APRILTAG_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct amdAprilTagsDetector_st* amdAprilTagsHandle;
typedef void* amdAprilTagsStream; /* hipStream_t */

typedef enum {
  AMDAT_SUCCESS = 0,
  AMDAT_INVALID_ARGUMENT = 1,
  AMDAT_UNSUPPORTED = 2,      /* tile size / family / encoding not supported */
  AMDAT_HIP_ERROR = 3,
  AMDAT_SIZE_MISMATCH = 4,    /* image size differs from the size given at creation */
  AMDAT_OUT_OF_MEMORY = 5,
  AMDAT_BATCH_TOO_LARGE = 6
} amdAprilTagsStatus;

/* Per-frame status bits reported by amdAprilTagsGetFrameFlags (capacity overflows are reported,
 * never undefined behaviour). */
#define AMDAT_FLAG_POINTS_OVERFLOW 0x1u    /* boundary points dropped */
#define AMDAT_FLAG_HASH_OVERFLOW 0x2u      /* cluster table full */
#define AMDAT_FLAG_CLUSTERS_OVERFLOW 0x4u  /* cluster list full */
#define AMDAT_FLAG_QUADS_OVERFLOW 0x8u     /* quad list full */
#define AMDAT_FLAG_DETS_OVERFLOW 0x10u     /* detection list full */

typedef enum {
  AMDAT_TAG36H11 = 0,   /* 587 codes (include/apriltag_amd_families.h states the provenance of every table) */
  AMDAT_TAG25H9 = 1,    /* 35 codes */
  AMDAT_TAG16H5 = 2,    /* 30 codes */
  AMDAT_TAG36H10 = 3,   /* no built-in table: the offline regeneration does not reproduce the published 2320 codes
                         * (include/apriltag_amd_families.h); the slot accepts a table through amdAprilTagsRegisterFamily */
  AMDAT_CUSTOM0 = 4,    /* slots filled by amdAprilTagsRegisterFamily[Ex] */
  AMDAT_CUSTOM1 = 5,
  AMDAT_CUSTOM2 = 6,
  AMDAT_CUSTOM3 = 7,
  AMDAT_CUSTOM4 = 8,
  AMDAT_ENUM_SIZE = 9
} amdAprilTagsFamily;

typedef struct {
  float fx, fy, cx, cy;
} amdAprilTagsCameraIntrinsics_t;

/* Pixel layout of the frames of a colour submission: the ROS encoding strings the reference accepts
 * (src/apriltag_node.cpp:76-82; its cuAprilTags branch takes rgb8 / bgr8 only, :469-476). */
typedef enum {
  AMDAT_ENC_MONO8 = 0,
  AMDAT_ENC_RGB8 = 1,
  AMDAT_ENC_BGR8 = 2,
  AMDAT_ENC_RGBA8 = 3,
  AMDAT_ENC_BGRA8 = 4,
  /* Raw formats, under their names in sensor_msgs/image_encodings: one sample per pixel, 8 bits or a
   * little-endian uint16.  A Bayer name lists the colours of pixels (0,0), (1,0) of row 0, then (0,1), (1,1) of row 1.  A submission of
   * such frames converts them to gray in one launch of its own, into a plane the handle owns, and is a mono8 submission from there on:
   * every record equals the record of the same handle given the converted plane as a mono8 frame (amdAprilTagsConvertRawToMono8 gives
   * that plane), with rectification, resize and every later stage on or off.  Taken by amdAprilTagsDetectBatchColor[Ex] and
   * amdAprilTagsSubmitBatchColor; the single-frame amdAprilTagsDetectColor keeps to the five values above.  The sample is the byte, or min(255, s >> shift) of a 16-bit
   * sample s (amdAprilTagsSetRawShift); mono16 is the sample; a Bayer frame is demosaiced bilinearly, its neighbours reflected about the
   * border, and turned into gray with the BT.601 weights of amdAprilTagsConvertToMono8.  A window into a Bayer image names the pattern at
   * the window's first pixel.  At submit, with nothing enqueued: AMDAT_INVALID_ARGUMENT for a pitch below bytes per sample x width and
   * for an odd pointer or pitch of a 16-bit encoding; AMDAT_SIZE_MISMATCH for a Bayer frame below 2 x 2; AMDAT_OUT_OF_MEMORY when the
   * plane could not be allocated. */
  AMDAT_ENC_BAYER_RGGB8 = 5,
  AMDAT_ENC_BAYER_BGGR8 = 6,
  AMDAT_ENC_BAYER_GBRG8 = 7,
  AMDAT_ENC_BAYER_GRBG8 = 8,
  AMDAT_ENC_MONO16 = 9,
  AMDAT_ENC_BAYER_RGGB16 = 10,
  AMDAT_ENC_BAYER_BGGR16 = 11,
  AMDAT_ENC_BAYER_GBRG16 = 12,
  AMDAT_ENC_BAYER_GRBG16 = 13
} amdAprilTagsEncoding;
/* "mono8", "rgb8", "bgr8", "rgba8", "bgra8", "bayer_rggb8", "bayer_bggr8", "bayer_gbrg8", "bayer_grbg8", "mono16", "bayer_rggb16",
 * "bayer_bggr16", "bayer_gbrg16", "bayer_grbg16" -> amdAprilTagsEncoding; -1 for any other string ("yuv422" among them). */
int amdAprilTagsEncodingFromName(const char* name);

/* Field NAMES follow cuAprilTagsImageInput_t as the reference assigns them (width, height, dev_ptr, pitch:
 * src/apriltag_node.cpp:481-486), so its binding compiles unchanged; the LAYOUT is this library's own (the closed header's
 * is not known), i.e. name-compatible, not binary-compatible, with cuAprilTags.  In the *Color calls dev_ptr is the
 * interleaved frame (the reference's uchar3*) and pitch its row stride in bytes. */
typedef struct {
  uint32_t width;
  uint32_t height;
  const uint8_t* dev_ptr; /* mono8 (or, in the *Color calls, interleaved colour), device memory */
  size_t pitch;           /* bytes per row; below 2^24, and pitch * height below 2^31 (AMDAT_INVALID_ARGUMENT otherwise) */
} amdAprilTagsImageInput_t;

typedef struct {
  float x, y;
} amdFloat2;

/* One detection.  The leading fields have the meaning the reference reads from cuAprilTagsID_t:
 * corners in the library's native order (= message order, src/apriltag_node.cpp:512-517; for an
 * upright tag: top-left, top-right, bottom-right, bottom-left), orientation COLUMN-major 3x3
 * (src/apriltag_node.cpp:416-419), translation in metres. */
typedef struct {
  uint16_t id;
  amdFloat2 corners[4];
  uint16_t hamming_error;
  float orientation[9];
  float translation[3];
  /* extensions */
  uint16_t family;        /* amdAprilTagsFamily */
  uint16_t reserved;
  float decision_margin;
  amdFloat2 center;       /* H(0,0); the reference recomputes it from the diagonals (:519-530) */
} amdAprilTagsID_t;

/* Full-precision record (parity tests, pose consumers): AprilRobotics conventions. */
typedef struct {
  int32_t family; /* index into the detector's family list */
  int32_t id;
  int32_t hamming;
  float decision_margin;
  double H[9];    /* row-major homography, tag [-1,1]^2 -> pixels */
  double c[2];    /* centre */
  double p[4][2]; /* H(-1,1), H(1,1), H(1,-1), H(-1,-1) */
  double R[9];    /* row-major rotation, tag frame in the camera optical frame */
  double t[3];    /* metres */
} amdAprilTagsDetectionEx_t;

typedef struct {
  uint32_t struct_size;        /* sizeof(amdAprilTagsConfig_t) of the header the caller was built against: set by
                                * amdAprilTagsDefaultConfig -- every configuration must start from that call.  Round 5's header is the
                                * FIRST versioned layout (struct_size went in at offset 0 then: a one-time ABI break against the
                                * rounds before it, which had no size field -- binaries built against those headers must be rebuilt;
                                * amdAprilTagsConfigLayoutVersion() says which layout a library speaks).  From that layout on the
                                * struct only grows at its end: a caller built against an older, shorter versioned header passes its
                                * smaller size and the fields it does not know keep their defaults (round 6 appended
                                * no_graph_replay and no_stream_priorities); a size below the first versioned layout's, or beyond the library's own, is
                                * AMDAT_INVALID_ARGUMENT (a struct that did not come from amdAprilTagsDefaultConfig). */
  uint32_t width, height;      /* input image size (fixed for the handle, as in the reference) */
  uint32_t tile_size;          /* 4 (src/apriltag_node.cpp:566) or 8; other values: AMDAT_UNSUPPORTED */
  uint32_t decimate;           /* quad_decimate, integer >= 1 (1 = cuAprilTags behaviour) */
  uint32_t num_families;       /* 1..4 */
  amdAprilTagsFamily families[4];
  amdAprilTagsCameraIntrinsics_t intrinsics;
  float tag_size;              /* metres (src/apriltag_node.cpp:565) */
  uint32_t max_batch;          /* frames per submission the handle is sized for (>= 1) */
  uint32_t refine_edges;       /* 1 */
  uint32_t max_hamming;        /* 2 */
  float decode_sharpening;     /* 0.25 */
  /* capacities per frame; 0 = defaults derived from the image size */
  uint32_t max_points;         /* boundary points; default 2 per working pixel */
  uint32_t hash_slots;         /* power of two */
  uint32_t max_clusters;       /* 0: starts at 65 536 and grows to the fullest frame's count when a frame fills it (up to one cluster per slot
                                * of the largest pair table); an explicit value is never grown and reports AMDAT_FLAG_CLUSTERS_OVERFLOW */
  uint32_t max_quads;          /* 0: starts at min(cluster capacity, 16 384) and doubles when a frame fills it; an explicit value is
                                * never grown and reports AMDAT_FLAG_QUADS_OVERFLOW */
  uint32_t max_detections;     /* 0: 1024 decoded candidates per frame (before the same-id overlap test), at most 65 535; not grown: a frame
                                * with more reports AMDAT_FLAG_DETS_OVERFLOW */
  int32_t device;              /* HIP device ordinal, -1 = current */
  float skew;                  /* K[0][1] of the pinhole matrix; 0 on the cuAprilTags-shaped path, the VPI path of
                                * the reference passes it with its 2x3 intrinsics (src/apriltag_node.cpp:215-225) */
  uint32_t corner_convention;  /* amdAprilTagsID_t only (amdAprilTagsDetectionEx_t always carries AprilRobotics' own):
                                * AMDAT_CORNERS_DEFAULT: corners[i] = p[3 - i], R as solved -- the reading of the reference's
                                * golden frame this library was built to (test/isaac_ros_apriltag_pol_test.py:132-175);
                                * AMDAT_CORNERS_ROTATED_180: the other reading of that frame -- corner index turned by two
                                * (corners[i] = p[(5 - i) & 3]) and the tag frame turned about its normal, R * Rz(pi) -- kept
                                * selectable until output of the closed library itself is available */
  uint32_t no_graph_replay;    /* != 0: small submissions are never stream-captured into launch graphs (plain enqueues, ~0.1 ms more per
                                * one-frame call).  For hosts whose OTHER threads make legacy-stream HIP calls (hipMemcpy, hipMemset on
                                * stream 0) on the same device while this handle detects: on ROCm 7 such a call fails -- in the host's
                                * thread -- whenever it meets a capture in progress, whatever the capture mode.  The
                                * library itself survives the collision either way (the submission goes out uncaptured). */
  uint32_t no_stream_priorities; /* != 0: a throughput-sized handle (max_batch > 8) creates its side streams without priorities (about
                                * 2 % fewer frames per second on 256-frame submissions).  For processes that ALSO hold handles of up to
                                * eight frames and create them AFTER the throughput-sized one: on ROCm 7 the launch graphs such a handle
                                * replays find their branches on the prioritised handle's hardware queues and run 30 % slower
                                * ("stream priorities").  Creating the small handles first, or one process per
                                * handle -- a node's shape -- needs nothing. */
} amdAprilTagsConfig_t;
#define AMDAT_CORNERS_DEFAULT 0u
#define AMDAT_CORNERS_ROTATED_180 1u

void amdAprilTagsDefaultConfig(amdAprilTagsConfig_t* cfg, uint32_t width, uint32_t height);
/* Layout generation of amdAprilTagsConfig_t this library was built with: 1 = the first versioned layout (struct_size at offset 0,
 * fields up to corner_convention), 2 = + no_graph_replay, 3 = + no_stream_priorities.  Layouts before 1 (no size field) are not
 * accepted. */
#define AMDAT_CONFIG_LAYOUT_VERSION 3
uint32_t amdAprilTagsConfigLayoutVersion(void);

/* nvCreateAprilTagsDetector-shaped constructor (one family, batch 1, decimate 1). */
int amdCreateAprilTagsDetector(amdAprilTagsHandle* handle, uint32_t img_width, uint32_t img_height,
                               uint32_t tile_size, amdAprilTagsFamily tag_family,
                               const amdAprilTagsCameraIntrinsics_t* cam, float tag_dim);
int amdCreateAprilTagsDetectorEx(amdAprilTagsHandle* handle, const amdAprilTagsConfig_t* cfg);
int amdAprilTagsDestroy(amdAprilTagsHandle handle);

/* cuAprilTagsDetect-shaped call: one frame, blocking. */
int amdAprilTagsDetect(amdAprilTagsHandle handle, const amdAprilTagsImageInput_t* img_input,
                       amdAprilTagsID_t* tags_out, uint32_t* num_tags, uint32_t max_tags,
                       amdAprilTagsStream stream);

/* The same call on a colour frame, as the reference's cuAprilTags branch makes it (uchar3 rgb8 / bgr8 device image,
 * src/apriltag_node.cpp:469-493): the gray value is the fixed-point BT.601 statement of amdAprilTagsConvertToMono8, formed by the
 * threshold pass's loader; results equal those of the mono8 call on the converted frame bit for bit.  encoding AMDAT_ENC_MONO8
 * is amdAprilTagsDetect.  This call keeps to the five encodings of the reference's table (AMDAT_UNSUPPORTED beyond AMDAT_ENC_BGRA8, as
 * before the raw formats existed); a Bayer or 16-bit frame goes through amdAprilTagsDetectBatchColor[Ex] or amdAprilTagsSubmitBatchColor
 * with n = 1. */
int amdAprilTagsDetectColor(amdAprilTagsHandle handle, const amdAprilTagsImageInput_t* img_input, amdAprilTagsEncoding encoding,
                            amdAprilTagsID_t* tags_out, uint32_t* num_tags, uint32_t max_tags, amdAprilTagsStream stream);

/* Batched call: n independent frames (n <= max_batch).  tags_out holds n*max_tags records,
 * num_tags n counts.  per_frame_intrinsics may be NULL (handle intrinsics used for all frames). */
int amdAprilTagsDetectBatch(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsImageInput_t* images,
                            const amdAprilTagsCameraIntrinsics_t* per_frame_intrinsics,
                            amdAprilTagsID_t* tags_out, uint32_t* num_tags, uint32_t max_tags,
                            amdAprilTagsStream stream);
/* Same, full-precision records. */
int amdAprilTagsDetectBatchEx(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsImageInput_t* images,
                              const amdAprilTagsCameraIntrinsics_t* per_frame_intrinsics,
                              amdAprilTagsDetectionEx_t* dets_out, uint32_t* num_dets, uint32_t max_dets,
                              amdAprilTagsStream stream);

/* The batched calls on colour frames (all frames of a submission share one encoding). */
int amdAprilTagsDetectBatchColor(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsImageInput_t* images,
                                 amdAprilTagsEncoding encoding, const amdAprilTagsCameraIntrinsics_t* per_frame_intrinsics,
                                 amdAprilTagsID_t* tags_out, uint32_t* num_tags, uint32_t max_tags, amdAprilTagsStream stream);
int amdAprilTagsDetectBatchColorEx(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsImageInput_t* images,
                                   amdAprilTagsEncoding encoding, const amdAprilTagsCameraIntrinsics_t* per_frame_intrinsics,
                                   amdAprilTagsDetectionEx_t* dets_out, uint32_t* num_dets, uint32_t max_dets,
                                   amdAprilTagsStream stream);

/* The batched call in two halves, for hosts that overlap the NEXT batch's host-to-device copy (on a stream of their own) with
 * this batch's detection: amdAprilTagsSubmitBatch enqueues the submission and returns; amdAprilTagsWaitBatch[Ex] blocks until
 * it is done and hands out the records (layout as amdAprilTagsDetectBatch[Ex] with the max_tags given at submit).  One
 * submission per handle at a time: a second Submit, or any other call that runs or inspects a submission, returns
 * AMDAT_INVALID_ARGUMENT until the wait has returned, and so does a wait with nothing in flight.  Images and their device
 * buffers must stay valid until the wait returns.  The blocking calls are exactly Submit followed by Wait. */
int amdAprilTagsSubmitBatch(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsImageInput_t* images,
                            const amdAprilTagsCameraIntrinsics_t* per_frame_intrinsics, uint32_t max_tags,
                            amdAprilTagsStream stream);
int amdAprilTagsSubmitBatchColor(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsImageInput_t* images,
                                 amdAprilTagsEncoding encoding, const amdAprilTagsCameraIntrinsics_t* per_frame_intrinsics,
                                 uint32_t max_tags, amdAprilTagsStream stream);
int amdAprilTagsWaitBatch(amdAprilTagsHandle handle, amdAprilTagsID_t* tags_out, uint32_t* num_tags);
int amdAprilTagsWaitBatchEx(amdAprilTagsHandle handle, amdAprilTagsDetectionEx_t* dets_out, uint32_t* num_dets);

/* Per-frame skew K[0][1] for the batch slots 0 .. n-1 of the submissions that follow (frames beyond n, and every frame after
 * n = 0, take the handle's amdAprilTagsConfig_t.skew).  The VPI path of the reference passes every camera's own skew with its
 * 2x3 intrinsics (src/apriltag_node.cpp:215-225); a batching front end that serves several cameras with one handle sets them
 * here next to the per-frame fx, fy, cx, cy of amdAprilTagsDetectBatch.  Only the pose depends on it. */
int amdAprilTagsSetFrameSkews(amdAprilTagsHandle handle, uint32_t n, const float* skews);

/* quad_sigma of AprilRobotics' detector (apriltag_ros: `blur` / `sigma`): a Gaussian blur (quad_sigma > 0) or sharpen (< 0) of the
 * working image ahead of the threshold, with upstream's integer taps.  At decimate 1 every stage reads the filtered
 * image; at decimate > 1 the threshold through the quad fit read the filtered decimated image, edge refinement and decode the unfiltered
 * frame.  The caller's buffers are never written.  |quad_sigma| < 0.5 is the identity: no filter (the default).  Callable whenever no
 * submission is in flight; takes effect with the next submission.  AMDAT_INVALID_ARGUMENT: null handle, NaN / inf, a submission in
 * flight; AMDAT_UNSUPPORTED: |quad_sigma| > 4; AMDAT_OUT_OF_MEMORY: the filtered plane (decimate 1) could not be allocated.  A refused
 * call leaves the previous setting in force.  A call that changes the filter (its taps, or on / off) retires the launch graphs the handle
 * has captured for small submissions; after 24 retired graphs in all (counting those of capacity growth and
 * cache evictions) the handle stops capturing new ones and enqueues such submissions plainly, about 0.1 ms more per one-frame call
 * (amdAprilTagsDebugGraphReplay reports it).  Set it once after create, or rarely. */
int amdAprilTagsSetQuadSigma(amdAprilTagsHandle handle, float quad_sigma);

/* Per-frame image sizes: mixed camera rigs and windows (regions of interest) in one submission.  Off (the default), every image of a
 * submission must have exactly the handle's width x height (AMDAT_SIZE_MISMATCH otherwise).  On, frame i is images[i].width x
 * images[i].height, any size with 1 <= width <= cfg.width, 1 <= height <= cfg.height whose working image (1 + (size - 1) / decimate
 * in each direction) has at least tile_size pixels both ways; a frame outside that range returns AMDAT_SIZE_MISMATCH with nothing
 * enqueued, and the pitch checks apply to every frame's own width.  The records of every frame are those of a handle of that
 * frame's size given that frame alone: everything the algorithm derives from the image size (tiles, bounds, the cluster-size cap,
 * quad_sigma's edge rules, the order of the records) follows the frame; memory, capacities and the launch schedule stay those of the
 * handle's size (DESIGN.md sections 3 and 4).  A window is a frame whose dev_ptr points at its first pixel inside a larger image and
 * whose pitch is that image's ("mixed rigs and windows").  Applies to every submitting call: Detect[Color],
 * DetectBatch[Color][Ex], SubmitBatch[Color] / WaitBatch[Ex], ThresholdOnly[Color].
 * Callable whenever no submission is in flight; AMDAT_INVALID_ARGUMENT: null handle, a submission in flight.  A call that changes
 * the mode retires the handle's captured launch graphs (the two modes differ in one launch), against the same budget of 24 retired
 * graphs as amdAprilTagsSetQuadSigma: set it once after create. */
int amdAprilTagsSetPerFrameSizes(amdAprilTagsHandle handle, int enable);

/* Rectification inside the submission: per-camera plumb_bob undistortion of every frame, batched, ahead of detection.
 * K, Knew: row-major 3x3; D = k1, k2, p1, p2, k3 (sensor_msgs/CameraInfo, distortion_model "plumb_bob"). */
typedef struct { double K[9]; double D[5]; double Knew[9]; } amdAprilTagsCameraModel_t;  /* row-major 3x3; plumb_bob */
/* ncams = 0 turns rectification off (the default: nothing changes).  Otherwise frame i of every following submission is first
 * undistorted with cams[i % ncams] -- one camera for every slot with ncams = 1, a camera per slot with ncams = n -- into a plane
 * the handle owns, and detected there: its records are exactly those of the same handle given the rectified frame R as a mono8 frame,
 * at every decimate, tile_size and quad_sigma.  R has the frame's own size w x h and R(x, y) is what amdAprilTagsRectifyMono8 computes
 * (the same double-precision projection, 1/32-pixel position, integer bilinear sum, 0 outside the source); a colour frame is first
 * turned into gray tap by tap with the fixed-point BT.601 weights of amdAprilTagsConvertToMono8, so R = rectify(convert(frame))
 * (DESIGN.md section 7b).  One launch per submission covers all frames; the caller's buffers are never written.
 * The library does NOT touch the pose intrinsics: the rectified image's camera is Knew, so pass {Knew[0], Knew[4], Knew[2], Knew[5]}
 * as per_frame_intrinsics (or in the handle's configuration), and Knew[1] through amdAprilTagsSetFrameSkews where it matters.
 * The models are host state of the handle, as the frame skews are, and travel to the device with each submission's descriptors: the
 * call makes no device synchronisation and a front end may call it before every flush.  The first call that turns rectification on
 * allocates the rectified plane (max_batch full-size mono8 frames).  Applies to every submitting call of this header -- Detect[Color],
 * DetectBatch[Color][Ex], SubmitBatch[Color] / WaitBatch[Ex] -- on both launch sets, and with amdAprilTagsSetPerFrameSizes on (each
 * frame's own width x height bounds its model; a window is rectified as the cropped array).  amdAprilTagsThresholdOnly[Color] of the
 * debug header never rectifies.
 * Callable whenever no submission is in flight.  AMDAT_INVALID_ARGUMENT: null handle, null cams with ncams > 0, ncams > max_batch, a
 * non-finite entry, Knew[0] == 0 or Knew[4] == 0, a submission in flight; AMDAT_OUT_OF_MEMORY: the plane could not be allocated.  A
 * refused call leaves the previous setting in force.  Turning the mode on or off retires the handle's captured launch graphs, against
 * the same budget of 24 as amdAprilTagsSetQuadSigma; changing only the models does not. */
int amdAprilTagsSetRectification(amdAprilTagsHandle handle, uint32_t ncams, const amdAprilTagsCameraModel_t* cams);

/* The same for every camera sensor_msgs/CameraInfo describes: its three distortion models, behind its rectification rotation R (the
 * one a stereo head fills in).  The values are those of amdAprilTagsDistortionFromName. */
typedef enum {
  AMDAT_DISTORTION_PLUMB_BOB = 0,             /* D = k1, k2, p1, p2, k3 */
  AMDAT_DISTORTION_RATIONAL_POLYNOMIAL = 1,   /* D = k1, k2, p1, p2, k3, k4, k5, k6 */
  AMDAT_DISTORTION_EQUIDISTANT = 2            /* D = k1, k2, k3, k4 (OpenCV's fisheye model) */
} amdAprilTagsDistortion;
/* "plumb_bob", "rational_polynomial", "equidistant" (CameraInfo.distortion_model) -> the enum; -1 for any other string or null. */
int amdAprilTagsDistortionFromName(const char* name);
/* K, R, Knew: row-major 3x3.  D: the kind's coefficients in CameraInfo's order; the entries beyond the kind's own must be 0. */
typedef struct { uint32_t kind; uint32_t reserved; double K[9]; double D[8]; double R[9]; double Knew[9]; } amdAprilTagsCameraModelEx_t;
/* amdAprilTagsSetRectification for cameras of any of the three kinds, with a rotation: the same contract, word for word -- host state
 * of the handle, no device synchronisation, cams[i % ncams] for frame i, one front launch per submission (one submission may mix kinds
 * and rotations), graphs retired only when the mode turns on or off, the same refusals, a refused call leaves the previous setting in
 * force -- and amdAprilTagsSetResize composes with it as with the other call: a tap of the resize is the rectified value under the
 * slot's model.  amdAprilTagsSetRectification is this call with AMDAT_DISTORTION_PLUMB_BOB and R = I; the later of the two calls holds.
 * Destination pixel (x, y) is projected as xp = (x - Knew[2]) / Knew[0], yp = (y - Knew[5]) / Knew[4], (X, Y, W) = R^T (xp, yp, 1),
 * xn = X / W, yn = Y / W (W <= 0: the pixel is 0), then through the kind's distortion and K, in double precision; position, bilinear
 * sum and bounds are those of amdAprilTagsRectifyMono8 (DESIGN.md section 7b has every operation).  A plumb_bob camera whose R is
 * exactly the identity gives what amdAprilTagsSetRectification gives, byte for byte, and so does rational_polynomial with k4 = k5 =
 * k6 = 0.
 * The pose intrinsics stay the caller's: pass Knew's fx, fy, cx, cy as with the other call.  R never touches the pose -- the tag pose
 * is reported in the RECTIFIED camera's frame, as it is behind a RectifyNode.
 * AMDAT_INVALID_ARGUMENT in addition to the other call's cases: a kind outside the enum, a non-finite entry of D or R, a non-zero
 * coefficient beyond the kind's own, and an R that is all zero -- a CameraInfo that was never filled in; the library does not guess,
 * a monocular camera passes the identity. */
int amdAprilTagsSetRectificationEx(amdAprilTagsHandle handle, uint32_t ncams, const amdAprilTagsCameraModelEx_t* cams);

/* Resize inside the submission, fused with the rectification where that is on: the reference's camera -> rectify -> resize -> AprilTag
 * graph as one submission. */
typedef struct { uint32_t width, height; } amdAprilTagsSize_t;
/* nsizes = 0 turns the resize off (the default: nothing changes).  Otherwise frame i of every following submission, whatever its own
 * size sw x sh (images[i].width / height: 1 .. 16384 each, larger or smaller than the handle's; beyond that AMDAT_SIZE_MISMATCH), is
 * first resized to sizes[i % nsizes] = dw x dh into a plane the handle owns, and detected there: its records are exactly those of the
 * same handle given the resized frame S as a mono8 frame, at every decimate, tile_size and quad_sigma.  S is what
 * amdAprilTagsResizeMono8 computes from the frame's gray plane G at the source size (oracle: ato_resize_mono8):
 * G = convert(frame) -- mono8 as it stands, colour through the BT.601 weights of amdAprilTagsConvertToMono8 -- or, with
 * amdAprilTagsSetRectification on, G = rectify(convert(frame)) with cams[i % ncams] and w = sw, h = sh.  With sw == dw and sh == dh
 * S == G.  One launch per submission covers all frames, writes the same plane rectification uses (the footprint grows by the
 * descriptors only), never writes the caller's buffers, and with rectification on never forms G in memory.
 * The TARGET size takes the place of the image size in every size rule: equal to the handle's size, or with
 * amdAprilTagsSetPerFrameSizes on any admissible size up to it; a violation is AMDAT_SIZE_MISMATCH at submit, with nothing enqueued.
 * The pitch rules apply to the source width.
 * The library does NOT touch the pose intrinsics.  The resized image's camera follows image_proc's convention: fx * dw / sw,
 * cx * dw / sw, fy * dh / sh, cy * dh / sh, and the skew * dw / sw; with rectification the same scaling applies to Knew.
 * The sizes are host state of the handle and travel with each submission's descriptors: no device synchronisation.  Applies to
 * Detect[Color], DetectBatch[Color][Ex], SubmitBatch[Color] / WaitBatch[Ex], on both launch sets; amdAprilTagsThresholdOnly[Color]
 * never resizes.
 * Callable whenever no submission is in flight.  AMDAT_INVALID_ARGUMENT: null handle, null sizes with nsizes > 0, nsizes > max_batch,
 * a zero dimension, a dimension above the handle's, a submission in flight; AMDAT_OUT_OF_MEMORY: the plane could not be allocated.  A
 * refused call leaves the previous setting in force.  Turning the mode on or off retires the handle's captured launch graphs, against
 * the same budget of 24 as amdAprilTagsSetQuadSigma; changing only the sizes does not. */
int amdAprilTagsSetResize(amdAprilTagsHandle handle, uint32_t nsizes, const amdAprilTagsSize_t* sizes);

/* Board pose inside the submission: tag bundles (apriltag_ros' word) solved per frame, behind the detector.
 * A bundle is a planar board: members (family_index, id, x, y, size) with the tag centre (x, y) on the board plane in metres, size the
 * black-border edge in metres (the meaning of tag_size) and the tag axes parallel to the board axes -- corner k of a record,
 * p[k] = H(c_k) with c = (-1, 1), (1, 1), (1, -1), (-1, -1), is the board point (x + size / 2 * c_k.x, y + size / 2 * c_k.y).
 * family_index indexes the handle's family list, as amdAprilTagsDetectionEx_t.family does.  Members turned in the plane and
 * non-planar bundles go through amdAprilTagsSetBundlesEx below. */
typedef struct { uint32_t family_index; uint32_t id; double x, y, size; } amdAprilTagsBundleMember_t;
typedef struct {
  const amdAprilTagsBundleMember_t* members;
  uint32_t nmembers;
  uint32_t max_hamming;          /* a record is used only if hamming <= max_hamming */
  float min_decision_margin;     /* ... and decision_margin >= min_decision_margin */
  uint32_t min_tags;             /* >= 1: with fewer used tags the bundle is not solved */
  char name[32];                 /* at most 31 characters and the terminator: the node shell's child frame is "bundle:<name>" */
} amdAprilTagsBundle_t;
#define AMDAT_BUNDLE_SOLVED 0u
#define AMDAT_BUNDLE_TOO_FEW_TAGS 1u
#define AMDAT_BUNDLE_SINGULAR 2u
#define AMDAT_MAX_BUNDLES 8u
#define AMDAT_MAX_BUNDLE_MEMBERS 1024u   /* over all bundles of a handle */
/* One record per (frame, bundle).  ntags: records used; nskipped: records of the bundle's members refused by a gate or by the
 * duplicate rule; R (row-major), t: the board frame in the camera frame, as a tag's; sq_err_sum: the sum of the squared pixel
 * reprojection errors of the 4 * ntags corners under (R, t, the frame's intrinsics and skew) -- no square root is taken: the RMS is
 * sqrt(sq_err_sum / (4 * ntags)).  A record whose status is not AMDAT_BUNDLE_SOLVED has R, t and sq_err_sum all zero. */
typedef struct { uint32_t bundle, status, ntags, nskipped; double R[9]; double t[3]; double sq_err_sum; } amdAprilTagsBundlePose_t;
/* nbundles = 0 turns the feature off (the default: nothing is launched or allocated).  Otherwise every following submission solves,
 * in one small launch behind the last detector stage, one pose per frame and bundle from ALL kept records of the frame (also those
 * beyond the caller's max_tags): one joint least-squares homography over the used tags' corners in normalised board and pixel
 * coordinates, normal equations in FP64 summed per record and then in record order, the 8 x 9 pivoted elimination of the single-tag
 * homography, and the single-tag pose routine (DESIGN.md section 7d has every operation; tests/bundle_ref.py states it in Python).
 * A (family, id) that occurs more than once among a frame's kept records contributes none of its records.  The records are in the
 * detected image's pixels and the intrinsics are the frame's, so the call composes with amdAprilTagsSetPerFrameSizes,
 * amdAprilTagsSetRectification[Ex] and amdAprilTagsSetResize as it stands.  Applies to Detect[Color], DetectBatch[Color][Ex] and
 * SubmitBatch[Color] / WaitBatch[Ex], on both launch sets.
 * Callable whenever no submission is in flight.  AMDAT_INVALID_ARGUMENT: null handle, null bundles with nbundles > 0, a null members
 * pointer or nmembers = 0, more than AMDAT_MAX_BUNDLES bundles or AMDAT_MAX_BUNDLE_MEMBERS members in all, a family_index outside the
 * handle's list, an id outside the family's codes, a (family_index, id) named twice (within or across bundles), a non-finite or
 * non-positive size, a non-finite coordinate, min_tags = 0, a name without terminator, a submission in flight; AMDAT_OUT_OF_MEMORY: the
 * device buffers could not be allocated.  A refused call leaves the previous setting in force.  Turning the mode on or off retires the
 * handle's captured launch graphs, against the same budget of 24 as amdAprilTagsSetQuadSigma; changing only the layout does not.
 * A bundle's max_hamming above 2147483646 (INT32_MAX - 1) is taken as that value, here and in amdAprilTagsSetBundlesEx: no decoded
 * record has a hamming above 3, and INT32_MAX itself is the mark of an invalid undistorted record (amdAprilTagsSetCornerUndistortion),
 * which no gate may pass. */
int amdAprilTagsSetBundles(amdAprilTagsHandle handle, uint32_t nbundles, const amdAprilTagsBundle_t* bundles);
/* The bundle records of the last completed submission: nframes x nbundles, frame-major (out[f * nbundles + b]).
 * AMDAT_INVALID_ARGUMENT: null handle or out, bundles off, nframes beyond the last submission's, a submission in flight. */
int amdAprilTagsGetBundlePoses(amdAprilTagsHandle handle, amdAprilTagsBundlePose_t* out, uint32_t nframes);

/* Rigid 3-D tag bundles: cubes, rigs and boards with turned tags, solved as one rigid body per frame inside the submission.
 * Every member carries a full pose in the bundle frame, as apriltag_ros' bundles do: R (row-major) and t give the TAG frame in the
 * BUNDLE frame, size is the black-border edge in metres.  Corner k of a record, p[k] = H(c_k) with the c_k of amdAprilTagsSetBundles,
 * is the bundle point R * (size / 2 * c_k.x, size / 2 * c_k.y, 0) + t.
 * R must be a rotation as it stands: a member with max |R R^T - I| > 1e-6 or det R <= 0 is refused; the library repairs nothing. */
typedef struct { uint32_t family_index; uint32_t id; double R[9]; double t[3]; double size; } amdAprilTagsBundleMemberEx_t;
#define AMDAT_MAX_RIGID_BUNDLE_MEMBERS 64u   /* per bundle: one lane of the solving wave holds one tag */
typedef struct {
  const amdAprilTagsBundleMemberEx_t* members;
  uint32_t nmembers;             /* 1 .. AMDAT_MAX_RIGID_BUNDLE_MEMBERS */
  uint32_t max_hamming;          /* the gates and min_tags of amdAprilTagsBundle_t */
  float min_decision_margin;
  uint32_t min_tags;
  uint32_t iterations;           /* 1 .. AMDAT_MAX_POSE_ITERATIONS steps of each of the two chains */
  char name[32];                 /* at most 31 characters and the terminator: the node shell's child frame is "bundle:<name>" */
} amdAprilTagsBundleEx_t;
#define AMDAT_BUNDLE_DEGENERATE 3u   /* both chains were degenerate: R, t are the seed start, err its E, everything else zero */
/* One record per (frame, bundle).  status: AMDAT_BUNDLE_SOLVED, AMDAT_BUNDLE_TOO_FEW_TAGS (every field behind nskipped zero) or
 * AMDAT_BUNDLE_DEGENERATE.  ntags, nskipped as amdAprilTagsBundlePose_t's.  seed: the index, in the frame's canonical order, of the
 * used record with the largest pixel area, whose homography pose starts both chains.  chosen: the chain R, t, err and sq_err_sum
 * come from (0: from the seed's homography pose, 1: from its mirror about the viewing ray); the other chain's result is in the
 * *_alt fields, which are zero where that chain was degenerate.  R (row-major), t: the bundle frame in the camera frame.  err:
 * the object-space error E = sum over the 4 * ntags corners of |(I - F_j)(R P_j + t)|^2 in square metres; sq_err_sum: the sum of
 * the squared pixel reprojection errors of the same corners, as amdAprilTagsBundlePose_t's. */
typedef struct {
  uint32_t bundle, status, ntags, nskipped, seed, chosen;
  double R[9], t[3], err, sq_err_sum;
  double R_alt[9], t_alt[3], err_alt, sq_err_sum_alt;
} amdAprilTagsBundlePoseEx_t;
/* nbundles = 0 turns the mode off (the default: nothing is launched or allocated).  Otherwise every following submission solves, in
 * one small launch behind the last detector stage, one pose per frame and bundle from ALL kept records of the frame: classification,
 * gates and the duplicate rule are amdAprilTagsSetBundles'; the pose is the object-space iteration of Lu, Hager and Mjolsness over
 * the 4 * ntags general 3-D points, run as two chains of `iterations` steps with no early exit, the lower E chosen and a tie going to
 * chain 0 (DESIGN.md section 7f has every operation; csrc/rigid_pose.h states it once for device and host, tests/rigid_bundle_ref.py
 * in Python).  A non-coplanar used set has one minimum; a coplanar one (a single face in view) keeps the planar two-fold ambiguity,
 * which the alternative reports.  FP64 throughout.  Composes with the other settings as amdAprilTagsSetBundles does, and runs beside
 * amdAprilTagsSetPoseRefinement.
 * The later of amdAprilTagsSetBundles / amdAprilTagsSetBundlesEx holds: one kind of bundle is on at a time, and turning one on
 * turns the other off.
 * Callable whenever no submission is in flight.  AMDAT_INVALID_ARGUMENT: everything amdAprilTagsSetBundles refuses (with the member
 * total bounded by AMDAT_MAX_BUNDLES * AMDAT_MAX_RIGID_BUNDLE_MEMBERS), more than AMDAT_MAX_RIGID_BUNDLE_MEMBERS members in a
 * bundle, a non-finite entry of R or t, an R with max |R R^T - I| > 1e-6 or det R <= 0, iterations = 0 or above
 * AMDAT_MAX_POSE_ITERATIONS; AMDAT_OUT_OF_MEMORY: the device buffers could not be allocated.  A refused call leaves the previous
 * setting in force.  A change of kind (planar <-> rigid) or on <-> off retires the handle's captured launch graphs, against the same
 * budget of 24 as amdAprilTagsSetQuadSigma; a change of layout, iteration count or gates does not (they live in device memory). */
int amdAprilTagsSetBundlesEx(amdAprilTagsHandle handle, uint32_t nbundles, const amdAprilTagsBundleEx_t* bundles);
/* The rigid bundle records of the last completed submission: nframes x nbundles, frame-major (out[f * nbundles + b]).
 * AMDAT_INVALID_ARGUMENT: null handle or out, the last submission did not run this mode, nframes beyond the last submission's, a
 * submission in flight. */
int amdAprilTagsGetBundlePosesEx(amdAprilTagsHandle handle, amdAprilTagsBundlePoseEx_t* out, uint32_t nframes);

/* Camera rigs: one pose per instant and rigid bundle from the tags ALL cameras of a calibrated rig saw at that instant, inside the
 * submission (DESIGN.md section 7j has every operation; csrc/rig_pose.h states it once for device and host, tests/rig_pose_ref.py in
 * Python).  A camera's extrinsics give the RIG frame in the CAMERA frame: X_cam = R X_rig + t, R row-major.  R must be a rotation as
 * it stands (the rule of amdAprilTagsBundleMemberEx_t). */
typedef struct { double R[9]; double t[3]; } amdAprilTagsRigCamera_t;
/* Batch slot i of a submission is camera `camera` of group `group`: the frames of one group were taken at one instant. */
typedef struct { uint32_t group; uint32_t camera; } amdAprilTagsRigSlot_t;
#define AMDAT_RIG_NO_CAMERA 0xFFFFFFFFu      /* the slot is detected as usual and belongs to no group */
#define AMDAT_MAX_RIG_CAMERAS 16u
#define AMDAT_MAX_RIG_OBSERVATIONS 64u   /* per (group, bundle): one lane of the solving wave holds one observation */
/* One record per (group, bundle).  An observation is one used record of one of the group's frames: the group's slots are walked in
 * ascending batch-slot order and each frame's kept records in their canonical order; classification, gates and the per-frame
 * duplicate rule are amdAprilTagsSetBundles' (a tag seen by two cameras is two observations).  nobs: the observations solved over,
 * at most AMDAT_MAX_RIG_OBSERVATIONS, which the bundle's min_tags gates; ndropped: the used records beyond them; nskipped: the
 * records a gate or the duplicate rule kept out, over all the group's frames; ncams: the distinct cameras among the nobs.
 * seed_frame, seed: the batch slot of the observation with the largest pixel area and its record's index in that frame's canonical
 * order; its homography pose, moved into the rig frame, starts both chains.  status, chosen and the *_alt fields as
 * amdAprilTagsBundlePoseEx_t's.  R (row-major), t: the bundle frame in the RIG frame.  err: the object-space error
 * E = sum |(I - F_j)(R P_j + t - o_j)|^2 over the 4 * nobs corners, F_j the projector onto the corner's viewing ray in the rig frame
 * and o_j its camera's centre; sq_err_sum: the squared pixel reprojection errors of the same corners, each under its own camera. */
typedef struct {
  uint32_t group, bundle, status, nobs, nskipped, ndropped, ncams, seed_frame, seed, chosen;
  double R[9], t[3], err, sq_err_sum;
  double R_alt[9], t_alt[3], err_alt, sq_err_sum_alt;
} amdAprilTagsRigBundlePose_t;
/* ncams = 0 turns the mode off (the default: nothing is launched or allocated, and no record of any other stage changes).  Otherwise
 * every following submission in which amdAprilTagsSetBundlesEx is on solves, in one small launch behind the other pose launches, one
 * pose per group and rigid bundle over all observations of the group's cameras at once: the object-space iteration of
 * amdAprilTagsSetBundlesEx with a ray origin per camera, two chains of the bundle's `iterations` steps, the same outcome rule.  The
 * per-frame rigid records are computed as before.  With amdAprilTagsSetBundlesEx off nothing is launched.  With
 * amdAprilTagsSetCornerUndistortion on the observations are the undistorted twins.  amdAprilTagsSetPoseCovariance leaves the rig
 * record alone.  The extrinsics are host state of the handle and travel with every submission's descriptors.
 * Callable whenever no submission is in flight.  AMDAT_INVALID_ARGUMENT: null handle, null cams with ncams > 0, ncams above
 * AMDAT_MAX_RIG_CAMERAS, a non-finite entry, an R with max |R R^T - I| > 1e-6 or det R <= 0, a submission in flight;
 * AMDAT_OUT_OF_MEMORY: the buffers could not be allocated.  A refused call leaves the previous setting in force.  Turning the mode
 * on or off retires the handle's captured launch graphs, against the same budget of 24 as amdAprilTagsSetQuadSigma; new extrinsics
 * do not. */
int amdAprilTagsSetRig(amdAprilTagsHandle handle, uint32_t ncams, const amdAprilTagsRigCamera_t* cams);
/* The slot map of the submissions that follow: slots[i] for batch slot i < n; a slot beyond n, and every slot where n = 0, follows
 * the default map: camera i % ncams of group i / ncams.  Host state, like the extrinsics: no graph is retired.
 * AMDAT_INVALID_ARGUMENT: null handle, null slots with n > 0, n above the handle's max_batch, a submission in flight.  While the rig
 * is on, a SUBMISSION is refused with AMDAT_INVALID_ARGUMENT, nothing enqueued, where a slot names a group index at or above its
 * frame count or a camera index at or above ncams (AMDAT_RIG_NO_CAMERA excepted), or where two slots name one (group, camera). */
int amdAprilTagsSetRigSlots(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsRigSlot_t* slots);
/* The rig records of the last completed submission: ngroups x nbundles, group-major (out[g * nbundles + b]), nbundles being
 * amdAprilTagsSetBundlesEx'.  Every group index below the submission's frame count has its records: a group no slot belongs to reads
 * AMDAT_BUNDLE_TOO_FEW_TAGS with zeros.  AMDAT_INVALID_ARGUMENT: null handle or out, the last submission did not run this mode (the
 * rig or the rigid bundles were off), ngroups beyond the last submission's frame count, a submission in flight. */
int amdAprilTagsGetRigBundlePoses(amdAprilTagsHandle handle, amdAprilTagsRigBundlePose_t* out, uint32_t ngroups);

/* Orthogonal-iteration tag pose with both minima, inside the submission (AprilRobotics' estimate_tag_pose: the object-space iteration
 * of Lu, Hager and Mjolsness from two starts, the lower error returned).  Off by default; amdAprilTagsID_t and
 * amdAprilTagsDetectionEx_t carry the homography pose whether it is on or off.
 * With the mode on, every following submission refines, in one small launch behind the last detector stage, the records it hands out
 * (the first min(kept, max_tags / max_dets) of every frame): two independent chains of `iterations` steps on the record's four corners
 * under the frame's intrinsics and skew and the handle's tag_size -- chain 0 from the record's homography pose (R_h, t_h), chain 1 from
 * its mirror about the viewing ray, (2 c c^T - I) R_h diag(-1, -1, 1) with c = t_h / |t_h|, the other minimum of the planar two-fold
 * ambiguity.  The chain with the smaller object-space error E is chosen, a tie goes to chain 0; the other is reported beside it, so
 * that a caller with a second view can decide otherwise.  DESIGN.md section 7e has every operation (csrc/pose_refine.h states it once
 * for device and host; tests/pose_refine_ref.py in Python).  FP64 throughout. */
#define AMDAT_POSE_REFINED 0u          /* both chains ran: R, t, err the chosen one's, R_alt, t_alt, err_alt the other's */
#define AMDAT_POSE_REFINED_NO_ALT 1u   /* chain 1 was degenerate: R, t, err are chain 0's, the alternative fields zero */
#define AMDAT_POSE_DEGENERATE 2u       /* chain 0 was degenerate: R, t the homography pose, err = err_homography, the alternative fields zero */
#define AMDAT_MAX_POSE_ITERATIONS 200u
/* chosen: the chain R, t come from (0 or 1).  R row-major, the tag frame in the camera frame, as a record's.  err, err_alt,
 * err_homography: E(R, t) = sum over the corners of |(I - F_k)(R P_k + t)|^2 in square metres, F_k the projector onto corner k's
 * viewing ray, P_k = tag_size / 2 * (c_k, 0); err_homography is E(R_h, t_h). */
typedef struct {
  uint32_t status, chosen;
  double R[9], t[3], err;
  double R_alt[9], t_alt[3], err_alt;
  double err_homography;
} amdAprilTagsRefinedPose_t;
/* iterations = 0 turns the mode off (the default: nothing is launched or allocated), 1 .. AMDAT_MAX_POSE_ITERATIONS turn it on;
 * upstream runs 50.  Applies to Detect[Color], DetectBatch[Color][Ex] and SubmitBatch[Color] / WaitBatch[Ex], on both launch sets;
 * ThresholdOnly never runs it.  Callable whenever no submission is in flight.  AMDAT_INVALID_ARGUMENT: null handle, iterations above
 * AMDAT_MAX_POSE_ITERATIONS, a submission in flight; AMDAT_OUT_OF_MEMORY: the record block could not be allocated.  A refused call
 * leaves the previous setting in force.  Turning the mode on or off retires the handle's captured launch graphs, against the same
 * budget of 24 as amdAprilTagsSetQuadSigma; changing only the count does not (it lives in device memory). */
int amdAprilTagsSetPoseRefinement(amdAprilTagsHandle handle, uint32_t iterations);
/* The refined poses of frame `frame` of the last completed submission: out[i] belongs to the i-th detection handed out for that frame;
 * their number through *n.  AMDAT_INVALID_ARGUMENT: null handle, out or n, the mode off in that submission, `frame` beyond its frames,
 * capacity below the frame's count (then *n still carries the count), a submission in flight. */
int amdAprilTagsGetRefinedPoses(amdAprilTagsHandle handle, uint32_t frame, amdAprilTagsRefinedPose_t* out, uint32_t capacity, uint32_t* n);

/* Pose covariance: a first-order 6 x 6 covariance for every pose amdAprilTagsSetPoseRefinement and amdAprilTagsSetBundlesEx hand out,
 * computed inside the same launches.  Off by default.
 * The parameters are those of ROS' geometry_msgs/PoseWithCovariance in the camera optical frame, x = (dt_x, dt_y, dt_z, dtheta_x,
 * dtheta_y, dtheta_z): the perturbed pose is t' = t + dt, R' = Exp(dtheta) R -- a rotation about axes parallel to the camera's,
 * through the tag or bundle origin; metres and radians, row-major, exactly symmetric.  The model: every corner coordinate carries
 * independent error of standard deviation corner_sigma_px, which is the CALLER's figure (nothing here estimates it);
 * cov = corner_sigma_px^2 (J^T J)^-1 with J the Jacobian of the pixel projection of the corners at the reported pose (DESIGN.md
 * section 7g has every operation; csrc/pose_covariance.h states it once for device and host, tests/pose_cov_ref.py in Python).
 * It is evaluated at the record's reported R, t whatever the status, and at R_alt, t_alt where an alternative exists.
 * valid: bit 0 cov, bit 1 cov_alt; a half whose bit is clear is 36 zeros (no alternative, a normal matrix that is not positive
 * definite in the arithmetic, a result that is not finite, a bundle with too few tags).
 * sq_err_sum, sq_err_sum_alt: for a tag, the sum over its four corners of the squared pixel reprojection error under R, t and under
 * R_alt, t_alt (zero without an alternative) -- what a caller can judge its sigma against; zero in a bundle's record, whose pose
 * record carries them. */
typedef struct {
  double cov[36], cov_alt[36];
  double sq_err_sum, sq_err_sum_alt;
  uint32_t valid, reserved;
} amdAprilTagsPoseCovariance_t;
/* corner_sigma_px = 0 turns the mode off (the default: nothing is launched or allocated, and no record changes by a bit), a finite
 * value > 0 turns it on.  The mode acts on whichever of amdAprilTagsSetPoseRefinement and amdAprilTagsSetBundlesEx is on in a
 * submission -- their launches run as their covariance instances; with neither on, nothing is launched.  Callable whenever no
 * submission is in flight.  AMDAT_INVALID_ARGUMENT: null handle, a NaN, an infinity or a negative value, a submission in flight;
 * AMDAT_OUT_OF_MEMORY: the record blocks could not be allocated.  A refused call leaves the previous setting in force.  Turning the
 * mode on or off retires the handle's captured launch graphs, against the same budget of 24 as amdAprilTagsSetQuadSigma; changing
 * only the value does not (its square lives in device memory). */
int amdAprilTagsSetPoseCovariance(amdAprilTagsHandle handle, double corner_sigma_px);
/* The covariance records beside amdAprilTagsGetRefinedPoses' records: same shape, same refusals, and refused where the last
 * submission did not run both modes. */
int amdAprilTagsGetRefinedPoseCovariances(amdAprilTagsHandle handle, uint32_t frame, amdAprilTagsPoseCovariance_t* out, uint32_t capacity, uint32_t* n);
/* The covariance records beside amdAprilTagsGetBundlePosesEx' records: same shape, same refusals, and refused where the last
 * submission did not run both modes. */
int amdAprilTagsGetBundlePoseCovariancesEx(amdAprilTagsHandle handle, amdAprilTagsPoseCovariance_t* out, uint32_t nframes);

/* Raw-frame mode: detect on the distorted frame as it comes from the camera and undistort the detected corners, not the pixels --
 * what a calibration or SLAM pipeline does with cv::undistortPoints.  Off by default; while it is off no record changes by a bit.
 * With the mode on, every following submission runs one small launch behind the last detector stage: every record the frame keeps
 * gets an undistorted twin under cams[i % ncams] for frame i.  Its corners are p_u[k] = undistort(p[k]) -- the raw pixel through
 * K^-1, the inverse of the kind's distortion by AMDAT_UNDISTORT_ITERATIONS Newton steps (no early exit), the rotation R and Knew; the
 * inverse, operation for operation, of the projection amdAprilTagsSetRectificationEx states.  Its H is the exact four-point homography
 * from the tag's corners c_k onto p_u[k], its c is H(0, 0), and its R, t are the homography pose under the frame's intrinsics and skew
 * and the handle's tag_size.  DESIGN.md section 7h has every operation (csrc/undistort.h states the point map once for device and
 * host; tests/undistort_ref.py in numpy).  FP64 throughout.
 * The records live in the coordinates a rectified image would have: pass Knew's fx, fy, cx, cy as the pose intrinsics, exactly as with
 * amdAprilTagsSetRectificationEx; with R set the pose is in the rectified camera's frame.  The model describes the DETECTED image: with
 * amdAprilTagsSetResize or a window of amdAprilTagsSetPerFrameSizes the caller scales or shifts K, as they do with the intrinsics.
 * amdAprilTagsID_t and amdAprilTagsDetectionEx_t keep the raw frame's values whether the mode is on or off; the bundle launches
 * (amdAprilTagsSetBundles, amdAprilTagsSetBundlesEx) and the refinement launch (amdAprilTagsSetPoseRefinement, with
 * amdAprilTagsSetPoseCovariance) read the undistorted twins in the raw records' place, so their poses are those of the ideal camera.
 * A record is AMDAT_UNDISTORT_INVALID where a corner does not come back to its pixel within 2^-20 px when pushed forward again (a
 * polynomial that folds over, a fisheye radius beyond the model's range), where a corner's ray points away from the rectified camera
 * (W <= 0), where a value is not finite, or where H is singular.  All geometric fields of such a record are zero; no bundle uses it
 * (it counts in nskipped, as a record that fails a gate), its refined pose is AMDAT_POSE_DEGENERATE with all other fields zero and
 * its covariance record is all zero with valid = 0.
 * Not covered: the detector itself is not distortion-aware (a strongly curved tag edge still meets a straight-line fit), the thin-prism
 * and tilted-sensor terms, and a skew in K or Knew (K[1], Knew[1] are not read). */
#define AMDAT_UNDISTORT_OK 0u
#define AMDAT_UNDISTORT_INVALID 1u
#define AMDAT_UNDISTORT_ITERATIONS 20
typedef struct {
  uint32_t status, reserved;
  double H[9], c[2], p[4][2], R[9], t[3];
} amdAprilTagsUndistortedDetection_t;
/* ncams = 0 turns the mode off.  The models are host state of the handle and travel to the device with each submission's descriptors:
 * no device synchronisation, a front end may call it before every flush.  The first call that turns the mode on allocates the twin
 * record list and the pinned record block.  Applies to every submitting call, on both launch sets.  Validation and refusals are those
 * of amdAprilTagsSetRectificationEx, and in addition: AMDAT_INVALID_ARGUMENT while rectification is on (a frame is either resampled or
 * read raw); amdAprilTagsSetRectification[Ex] with ncams > 0 is refused while this mode is on.  A refused call
 * leaves the previous setting in force.  Turning the mode on or off retires the handle's captured launch graphs, against the same
 * budget of 24 as amdAprilTagsSetQuadSigma; changing only the models does not. */
int amdAprilTagsSetCornerUndistortion(amdAprilTagsHandle handle, uint32_t ncams, const amdAprilTagsCameraModelEx_t* cams);
/* The undistorted records of frame `frame` of the last completed submission: out[i] belongs to the i-th detection handed out for that
 * frame; their number through *n.  The shape and the refusals of amdAprilTagsGetRefinedPoses. */
int amdAprilTagsGetUndistortedDetections(amdAprilTagsHandle handle, uint32_t frame, amdAprilTagsUndistortedDetection_t* out, uint32_t capacity, uint32_t* n);

/* ---- The tag table: which tags a deployment has and how big each one is (apriltag_ros: standalone_tags; ROS 2 apriltag_ros: tag.ids /
 * tag.sizes).  Without a table every tag has the handle's tag_size and every decoded tag is reported.  An entry gives tag `id` of
 * family families[family_index] of the handle's configuration the edge `size` in metres; id AMDAT_TAG_ID_ANY stands for every id of
 * that family that has no entry of its own, and size 0 for the handle's tag_size ("listed, at the default size").  The record's pose
 * (R, t of amdAprilTagsDetectionEx_t), the pose of its undistorted twin, its refined pose and its covariance are those of a tag of
 * its own size: exactly what a handle with that tag_size reports for the record.  Bundles are not touched: their members carry
 * sizes of their own.
 * listed_only = 1: a decoded tag that the table does not list is dropped ahead of the cut to max_tags, like a duplicate: it is in no
 * count, no record list and no stage behind (twins, bundles, rigs, refined poses, covariances); AMDAT_FLAG_DETS_OVERFLOW and the
 * AMDAT_DBG_DETS buffer still speak of the records before that.  The members of configured bundles are NOT listed implicitly: with
 * listed_only they must be in the table, or the bundles never see them.
 * n = 0 turns the table off and frees its device buffer (49 168 bytes, allocated by the first call with n > 0).  Entries, count and
 * flag live in device memory: changing them retires no captured launch graph; only setting a table where there was none, or
 * turning it off, does (against the same budget of 24 as amdAprilTagsSetQuadSigma).  Takes effect with the next submission.
 * AMDAT_INVALID_ARGUMENT, with the previous table left in force and no graph retired: a null handle, n > 0 with entries == NULL,
 * n > AMDAT_MAX_TAG_ENTRIES, listed_only > 1, a non-zero reserved, a family_index at or beyond the handle's family count, an id at
 * or beyond the family's code count other than AMDAT_TAG_ID_ANY, a negative or non-finite size, two entries for one (family_index,
 * id), a submission in flight. */
#define AMDAT_MAX_TAG_ENTRIES 4096u
#define AMDAT_TAG_ID_ANY 0xFFFFu
typedef struct {
  uint32_t family_index;
  uint32_t id;
  float size;
  uint32_t reserved;
} amdAprilTagsTagEntry_t;
int amdAprilTagsSetTagTable(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsTagEntry_t* entries, uint32_t listed_only);

/* Device memory the handle owns, in bytes. */
int amdAprilTagsGetDeviceBytes(amdAprilTagsHandle handle, size_t* bytes);

/* Status bits of the frames of the last submission (n values). */
int amdAprilTagsGetFrameFlags(amdAprilTagsHandle handle, uint32_t* flags, uint32_t n);

/* Colour -> mono8 on the device.  encoding: "mono8","rgb8","bgr8","rgba8","bgra8"
 * (src/apriltag_node.cpp:76-82), or a raw format's name (amdAprilTagsConvertRawToMono8 at shift 8). */
int amdAprilTagsConvertToMono8(const void* src_dev, size_t src_pitch, const char* encoding, uint32_t width,
                               uint32_t height, uint8_t* dst_dev, size_t dst_pitch, amdAprilTagsStream stream);

/* The same for the raw formats (AMDAT_ENC_BAYER_RGGB8 .. AMDAT_ENC_BAYER_GRBG16), which amdAprilTagsConvertToMono8 takes by name at
 * shift 8: the plane a submission of such frames detects on.  shift: 0 .. 8, read by the 16-bit encodings.  dst at any address and
 * pitch >= width; src at any address and pitch for 8-bit samples, both even for 16-bit ones.  AMDAT_UNSUPPORTED: another encoding;
 * AMDAT_SIZE_MISMATCH: a Bayer frame below 2 x 2, a dimension above 16384; AMDAT_INVALID_ARGUMENT otherwise. */
int amdAprilTagsConvertRawToMono8(const void* src_dev, size_t src_pitch, amdAprilTagsEncoding encoding, uint32_t shift, uint32_t width,
                                  uint32_t height, uint8_t* dst_dev, size_t dst_pitch, amdAprilTagsStream stream);
/* The shift of the 16-bit encodings' samples for the handle's submissions: 0 .. 8, default 8 (the high byte); a sensor with 12
 * significant bits sets 4.  Host state that travels with the submission's descriptors: no captured launch sequence is retired.
 * AMDAT_INVALID_ARGUMENT: a null handle, shift > 8, a submission in flight. */
int amdAprilTagsSetRawShift(amdAprilTagsHandle handle, uint32_t shift);

/* ---- front steps of the usual graph (camera -> rectify -> resize -> apriltag; reference README.md:16-29,
 * launch/isaac_ros_apriltag_usb_cam.launch.py:43-63) on mono8 device images ------------------------- */
/* Bilinear resize, pixel-centre aligned; source coordinates and weights are 1/2048 fixed point, so the
 * result is exactly reproducible (oracle: ato_resize_mono8). */
int amdAprilTagsResizeMono8(const uint8_t* src_dev, size_t src_pitch, uint32_t src_width, uint32_t src_height,
                            uint8_t* dst_dev, size_t dst_pitch, uint32_t dst_width, uint32_t dst_height,
                            amdAprilTagsStream stream);
/* Undistortion of a plumb_bob image (sensor_msgs/CameraInfo K and D = k1,k2,p1,p2,k3) onto the pinhole
 * camera K_new (row-major 3x3 each): every destination pixel is projected through the distortion model
 * in double precision, the source position is quantised to 1/32 pixel and sampled bilinearly in integer
 * arithmetic; pixels that map outside the source are 0 (oracle: ato_rectify_mono8).  One frame per call on the
 * caller's stream; amdAprilTagsSetRectification does the same inside the submission, for every frame at once. */
int amdAprilTagsRectifyMono8(const uint8_t* src_dev, size_t src_pitch, uint8_t* dst_dev, size_t dst_pitch, uint32_t width,
                             uint32_t height, const double* K9, const double* D5, const double* Knew9,
                             amdAprilTagsStream stream);
/* The same for a camera of any of the three kinds with a rotation (amdAprilTagsCameraModelEx_t, validated as by
 * amdAprilTagsSetRectificationEx): what that call computes inside the submission, for one mono8 frame on the caller's stream. */
int amdAprilTagsRectifyMono8Ex(const uint8_t* src_dev, size_t src_pitch, uint8_t* dst_dev, size_t dst_pitch, uint32_t width,
                               uint32_t height, const amdAprilTagsCameraModelEx_t* cam, amdAprilTagsStream stream);

/* Device-memory helpers for hosts that do not link the HIP runtime themselves (the node shell copies
 * sensor_msgs/Image payloads with these).  Plain hipMalloc / hipFree / hipMemcpyAsync + sync. */
int amdAprilTagsDeviceAlloc(void** dev_ptr, size_t bytes);
int amdAprilTagsDeviceFree(void* dev_ptr);
int amdAprilTagsCopyToDevice(void* dst_dev, const void* src_host, size_t bytes, amdAprilTagsStream stream);
/* Enqueue-only form on a stream of the host's (amdAprilTagsStreamCreate): the copy is ordered ahead of a detection submitted on the
 * same stream, whose wait then covers both; the source must stay valid until that detection has returned. */
int amdAprilTagsCopyToDeviceAsync(void* dst_dev, const void* src_host, size_t bytes, amdAprilTagsStream stream);
int amdAprilTagsStreamCreate(amdAprilTagsStream* stream);    /* a non-blocking HIP stream */
int amdAprilTagsStreamDestroy(amdAprilTagsStream stream);   /* waits for it first */

/* Registers a tag family as data (row-major codes, MSB = top-left data cell) in a custom slot. */
int amdAprilTagsRegisterFamily(amdAprilTagsFamily slot, const char* name, uint32_t data_bits_per_side,
                               const uint64_t* codes, uint32_t ncodes);
/* The same for an AprilTag-3 style layout -- what the circle / standard / custom families of the reference's table
 * (src/apriltag_node.cpp:47-58: circle21h7, circle49h12, custom48h12, standard41h12, standard52h13) need: nbits data bits
 * (<= 64), bit i at cell (bit_x[i], bit_y[i]) in border coordinates ((0, 0) = top-left cell of the border square of
 * width_at_border cells, 3 <= width_at_border <= 10: the decode kernel holds 8 x 10 border samples, and a classic 8 x 8
 * family, the widest 64-bit word, needs exactly 10; cells of outer rings are negative or >= width_at_border), total_width
 * cells across everything (<= 12, same parity as width_at_border), reversed_border != 0 when the border square is white inside a black ring.
 * Bit (nbits - 1 - i) of a code is data bit i (AprilTag 3's own convention), 1 = white.  The layout must map onto itself
 * under the quarter turn (x, y) -> (width_at_border - 1 - y, x); AMDAT_INVALID_ARGUMENT otherwise.  This library ships
 * no code tables for those five families (none can be verified offline); a host that has them registers them here under
 * the reference's names and amdAprilTagsFamilyFromName / the node shell find them. */
int amdAprilTagsRegisterFamilyEx(amdAprilTagsFamily slot, const char* name, uint32_t nbits, const int8_t* bit_x,
                                 const int8_t* bit_y, uint32_t width_at_border, uint32_t total_width, int reversed_border,
                                 const uint64_t* codes, uint32_t ncodes);
/* Registered names are at most 31 characters and code words carry no bits above the family's width (AMDAT_INVALID_ARGUMENT
 * otherwise).  amdAprilTagsUnregisterFamily empties a registrable slot again (handles created earlier keep their copy of the
 * table). */
int amdAprilTagsUnregisterFamily(amdAprilTagsFamily slot);
/* Family metadata: returns 0 and fills the outputs if the family is known.  The pointers stay valid until the slot is
 * registered again or emptied. */
int amdAprilTagsFamilyInfo(amdAprilTagsFamily family, const char** name, uint32_t* data_bits_per_side,
                           uint32_t* ncodes, const uint64_t** codes);
/* Family lookup by the reference's parameter string (src/apriltag_node.cpp:47-58); -1 if unknown
 * or without an offline codebook. */
int amdAprilTagsFamilyFromName(const char* name);

/* Measurement and stage-inspection entry points (profiling, the threshold-only launch of the roofline measurement,
 * intermediate buffers, the device arithmetic self check) are declared in apriltag_amd_debug.h: they are exported by
 * the same library but are not part of the detector boundary a node binds. */

#ifdef __cplusplus
}
#endif
#endif /* APRILTAG_AMD_H_ */
