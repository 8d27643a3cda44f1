// detector.hip -- host side of libapriltag_amd.so: the C ABI declared in include/apriltag_amd.h,
// buffer management, and the launch sequence of one batched submission.
//
// Replaces the closed cuAprilTags calls of the reference node
// (src/apriltag_node.cpp:450-452 create, :491-493 detect, :556 destroy).  gfx950 only.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/apriltag_amd.h"
#include "../../include/apriltag_amd_debug.h"
#include "../../include/apriltag_amd_families.h"
#include "common.h"
#include "kernels_bundle.h"
#include "kernels_rigid.h"
#include "kernels_rig.h"
#include "kernels_cc.h"
#include "kernels_cluster.h"
#include "kernels_decode.h"
#include "kernels_decode_wave.h"
#include "kernels_filter.h"
#include "kernels_frontend.h"
#include "kernels_pose.h"
#include "kernels_quad.h"
#include "kernels_quad_small.h"
#include "kernels_raw.h"
#include "kernels_threshold.h"
#include "kernels_undistort.h"
#include "launch_plan.h"
#include "post_plan.h"

static_assert(sizeof(DetRec) == sizeof(amdAprilTagsDetectionEx_t), "DetRec must match the public record");
static_assert(sizeof(QuadRec) == 48, "QuadRec layout");
static_assert(sizeof(ClusterRec) == 16, "ClusterRec layout");

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) {                                                                        \
      fprintf(stderr, "[apriltag_amd] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return AMDAT_HIP_ERROR;                                                                      \
    }                                                                                              \
  } while (0)

// ------------------------------------------------------------------------------------------------
// family registry
// ------------------------------------------------------------------------------------------------
namespace {
struct FamilyHost {
  const char* name = nullptr;
  uint32_t d = 0;            // data cells per side of a classic family, 0 for other layouts
  uint32_t nbits = 0, width_at_border = 0, total_width = 0;
  int reversed_border = 0;
  int8_t bit_x[64] = {0}, bit_y[64] = {0};
  uint8_t rot_src[64] = {0};
  uint32_t ncodes = 0;
  const uint64_t* codes = nullptr;
  std::vector<uint64_t> owned;
  char name_buf[32] = {0};
};
// Fills the rotation table; false if the layout does not map onto itself under (x, y) -> (wb - 1 - y, x) or repeats a cell.
bool family_finish_layout(FamilyHost& f) {
  for (uint32_t i = 0; i < f.nbits; i++) {
    const int sx = (int)f.width_at_border - 1 - f.bit_y[i], sy = f.bit_x[i];
    int src = -1;
    for (uint32_t j = 0; j < f.nbits; j++) {
      if (f.bit_x[j] == sx && f.bit_y[j] == sy) src = (int)j;
      if (j < i && f.bit_x[j] == f.bit_x[i] && f.bit_y[j] == f.bit_y[i]) return false;
    }
    if (src < 0) return false;
    f.rot_src[i] = (uint8_t)src;
  }
  return true;
}
void family_set_classic(FamilyHost& f, uint32_t d) {
  f.d = d; f.nbits = d * d; f.width_at_border = d + 2; f.total_width = d + 4; f.reversed_border = 0;
  for (uint32_t i = 0; i < f.nbits; i++) { f.bit_x[i] = (int8_t)(1 + i % d); f.bit_y[i] = (int8_t)(1 + i / d); }
  family_finish_layout(f);
}
FamilyHost g_families[AMDAT_ENUM_SIZE];
std::once_flag g_fam_once;
std::mutex g_fam_mutex;

void init_families() {
  g_families[AMDAT_TAG36H11].name = "tag36h11";
  family_set_classic(g_families[AMDAT_TAG36H11], 6);
  g_families[AMDAT_TAG36H11].ncodes = APRILTAG_AMD_TAG36H11_NCODES;
  g_families[AMDAT_TAG36H11].codes = apriltag_amd_tag36h11_codes;
  g_families[AMDAT_TAG25H9].name = "tag25h9";
  family_set_classic(g_families[AMDAT_TAG25H9], 5);
  g_families[AMDAT_TAG25H9].ncodes = APRILTAG_AMD_TAG25H9_NCODES;
  g_families[AMDAT_TAG25H9].codes = apriltag_amd_tag25h9_codes;
  g_families[AMDAT_TAG16H5].name = "tag16h5";
  family_set_classic(g_families[AMDAT_TAG16H5], 4);
  g_families[AMDAT_TAG16H5].ncodes = APRILTAG_AMD_TAG16H5_NCODES;
  g_families[AMDAT_TAG16H5].codes = apriltag_amd_tag16h5_codes;
  // (AMDAT_TAG36H10 starts empty: see the header)
}

bool is_registrable_slot(int slot) { return slot == AMDAT_TAG36H10 || (slot >= AMDAT_CUSTOM0 && slot < AMDAT_ENUM_SIZE); }

// roctx ranges around the stages, behind the profiling switch: the marker library is looked up at run
// time the first time profiling is on (libroctx64.so ships with ROCm; a host without it simply gets no ranges), so the
// product library has no link-time dependency on the tracing stack and an unprofiled call never touches it.
struct RoctxApi {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  RoctxApi() {
    void* h = dlopen("libroctx64.so", RTLD_LAZY | RTLD_LOCAL);
    if (!h) h = dlopen("libroctx64.so.4", RTLD_LAZY | RTLD_LOCAL);
    if (!h) return;
    push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
    pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
    if (!push || !pop) { push = nullptr; pop = nullptr; }
  }
};
static const RoctxApi& roctx() { static const RoctxApi api; return api; }

const char* kStageNames[AMDAT_NUM_STAGES] = {"upload_clear", "threshold", "cc_local",  "cc_border",
                                             "cc_sizes",   "points",    "cluster_select", "scatter",
                                             "fit_quads",    "decode",    "reconcile", "download"};

// Makes `device` current for the scope of one C-ABI call and restores the caller's device afterwards, so
// that a multi-GPU host (one handle per device in one process) never finds its current device changed.
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) ok = hipSetDevice(device) == hipSuccess; else prev = -1;
  }
  ~DeviceGuard() { if (prev >= 0) hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

uint32_t next_pow2(uint32_t v) {
  uint32_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

// A device allocation the handle owns: its pointer and the bytes device_bytes counts for it (dev_alloc / dev_free).
struct DevAlloc {
  void* p = nullptr;
  size_t bytes = 0;
};
template <class T> struct DevBuf : DevAlloc {
  operator T*() const { return static_cast<T*>(p); }
};
// A pinned host block the handle owns (host_alloc); free_all releases every one that was allocated.
struct HostAlloc {
  void* p = nullptr;
};
template <class T> struct HostBuf : HostAlloc {
  operator T*() const { return static_cast<T*>(p); }
};
}  // namespace

// Scratch of one k_fit_quads class (launch_plan.h: FqClassSpec); k_fit_small keeps its moments in LDS and has none.
struct FqScratch {
  DevBuf<double> d_lf;                    // grid x slot_cap x 6 doubles
  DevBuf<double> d_errs;                  // grid x slot_cap x 2 doubles: error arrays of clusters that exceed what the
                                          // kernel keeps in LDS / registers (slot_cap > 16 x nt, or > sort_cap)
};

struct amdAprilTagsDetector_st {
  amdAprilTagsConfig_t cfg;
  DetParams P;
  int device = 0;
  int num_cus = 256;
  size_t device_bytes = 0;
  hipStream_t own_stream = nullptr;
  // the size classes of the quad fit fork to auxiliary streams and join before decode
  hipStream_t aux_stream[FQ_NAUX] = {};
  bool aux_prioritised = false;      // the side streams carry priorities (handles above eight frames per submission; see creation)
  hipEvent_t ev_fork = nullptr, ev_join[FQ_NAUX] = {};
  // device buffers
  DevBuf<uint8_t> d_gray;             // working-size gray plane: decimated handles, and (allocated on first use) colour submissions and
                                      // the quad_sigma filter at decimate 1
  DevBuf<uint8_t> d_conv;             // full-size mono8 plane of colour submissions that take the conversion launch (decimate > 1, tile_size 8)
  size_t conv_pitch = 0;
  DevBuf<uint8_t> d_thr;
  DevBuf<uint8_t> d_tmin;            // per-tile min / max of the two-pass threshold (tile_size != 4 only)
  DevBuf<uint8_t> d_tmax;
  DevBuf<uint32_t> d_label;
  DevBuf<uint32_t> d_csize;
  DevBuf<uint32_t> d_roots;
  DevBuf<uint32_t> d_perim;          // tile perimeters (class + tile-local root per pixel), k_cc_local -> k_cc_border (kernels_cc.h: CcPerim)
  DevBuf<unsigned long long> d_hkeys;
  DevBuf<uint32_t> d_hcnt;
  DevBuf<uint32_t> d_hoff;
  DevBuf<uint32_t> d_stage;          // one word per staged boundary point (kernels_cluster.h, pass 3 of k_points)
  DevBuf<uint2> d_bhdr;              // per block (tile) of k_points: {first staging word, words}
  DevBuf<uint2> d_btab;              // per block: its component-pair table, {pair-table slot, base rank inside the cluster} per entry
  DevBuf<uint4> d_long;              // {slot, rank, packed point}: emissions without a block-table entry
  DevBuf<uint32_t> d_pts;
  DevBuf<ClusterRec> d_clusters;
  DevBuf<uint32_t> d_work;           // work lists of the quad fit (all classes, FqWorkLayout)
  bool tables_dirty = false;         // a submission was cut short after k_points: the pair table is not empty
  DevBuf<uint32_t> d_workctl;        // [0..7] items per class, [8..15] pop cursors, [16..23] items per class after k_fit_prefilter, [24] the prefilter's own cursor
  DevBuf<uint32_t> d_work2;          // compact work lists of the prefiltered classes (same layout as d_work)
  DevBuf<unsigned long long> d_keys_scr;     // only when a cluster can exceed the LDS key array (large images)
  DevBuf<QuadRec> d_quads;
  DevBuf<DetRec> d_dets;
  DevBuf<uint16_t> d_order;
  DevBuf<FitCand> d_cands;           // quad candidates of k_fit_quads (four lines each), consumed by k_quad_finish
  FrameCounters* d_counters = nullptr;
  DevBuf<FrameDesc> d_frames;
  DevBuf<uint64_t> d_codes[AT_MAX_FAMILIES];
  std::vector<DevAlloc*> owned;      // every holder above that has had an allocation (dev_alloc): what free_all releases
  unsigned long long* d_ptprof = nullptr;  // per-phase cycle counters of k_points (same builds), inside d_fqprof's allocation
  DevBuf<unsigned long long> d_fqprof;     // per-phase cycle counters of k_fit_quads (-DAMDAT_FQ_PROFILE builds only)
  FqClassTable fq;                   // size classes of the quad fit (launch_plan.h; set at creation)
  FqScratch fq_scratch[FQ_NCLS];
  FqWorkLayouts work_layout;         // their work lists on either launch set (alloc_point_buffers)
  GrowLimits grow = {};              // which capacities follow the content, and up to what (growth.h; set at creation)
  bool pending_hash_grow = false;    // the last submission crowded the pair table: it grows before the next one (begin_batch)
  uint32_t lcap_div = 0;             // long-record capacity = point capacity / lcap_div (alloc_point_buffers; halves when the long records overflow)
  bool unusable = false;             // a capacity change failed twice (grown and original size): buffers are gone, every later call reports it
  // pinned host buffers
  HostBuf<FrameDesc> h_frames;
  HostBuf<FrameCounters> h_counters;
  HostBuf<DetRec> h_out;
  std::vector<HostAlloc*> host_owned;   // every pinned holder that has had an allocation (host_alloc): what free_all releases
  // profiling
  bool profiling = false;
  bool fq_counters = false;  // per-phase cycle counters inside k_fit_quads (profiling level 2; perturbs timing)
  bool fq_attr_set = false;
  // captured enqueue sequence of small submissions (see run_batch)
  uint32_t graph_max_frames = 8;
  struct GraphEntry { hipGraphExec_t exec = nullptr; uint32_t n = 0, ostride = 0, fmt = 0; hipStream_t stream = nullptr; uint64_t last_use = 0;
                      bool general = false;      // general: captured with the general front kernel (rect_general)
                      uint32_t raw = 0;          // raw: captured with the raw conversion launch of that instance in front (RAW_KIND_*; fmt is mono8 then)
                      uint32_t nodes = 0; };     // the graph's nodes (amdAprilTagsDebugLastGraphNodes)
  GraphEntry graphs[6];
  std::vector<hipGraphExec_t> retired_graphs;   // see drop_graphs
  uint64_t graph_clock = 0;
  uint32_t graph_misses = 0;         // consecutive captures that had to evict an entry
  uint32_t last_graph_nodes = 0;     // nodes of the graph the last launch replayed; 0: plain enqueues
  uint32_t capture_failures = 0;     // captures that did not end in a graph (recover_from_failed_capture)
  hipEvent_t ev[AMDAT_NUM_STAGES + 1] = {};
  // which launch set a submission gets: by its size (AMDAT_PATH_AUTO) or pinned by amdAprilTagsDebugSetSubmissionPath, so that
  // the parity tests can put BOTH launch sets under the oracle at any frame count
  bool events_recorded = false;      // the submission in flight recorded the stage events (profiling on, no graph replay)
  struct { bool active = false; uint32_t n = 0, ostride = 0, max_out = 0; hipStream_t stream = nullptr; } inflight;   // amdAprilTagsSubmitBatch .. WaitBatch
  std::vector<float> frame_skew;     // per batch slot, amdAprilTagsSetFrameSkews; empty: cfg.skew for every frame
  uint32_t launched_n = 0;
  uint32_t launched_fmt = 0;         // amdAprilTagsEncoding of the submission in flight (a regrowth relaunch repeats it)
  uint32_t seq = 0;                  // launch counter: travels through the descriptor block and comes back with the counters
  uint32_t late_waits = 0;           // launches whose stream wait returned before their results (finish_once); amdAprilTagsDebugLateWaits
  int path_mode = AMDAT_PATH_AUTO;
  int last_path = AMDAT_PATH_AUTO;   // the set the last submission ran (amdAprilTagsDebugLastSubmissionPath)
  float stage_ms[AMDAT_NUM_STAGES] = {};
  // The stages behind k_reconcile (post_plan.h).  `post` is what the setters set, and they refuse while a
  // submission is in flight; `last` is what the last submission ran with, assigned once by begin_batch and emptied by the entry
  // points that never run the back end: all that the getters, the stamp check and the launches themselves read.
  PostMode post;
  struct LastSubmission {
    uint32_t n = 0, ostride = 0;   // frames, and record slots per frame
    PostMode post;
    bool rectified = false;        // it formed the rectified plane (AMDAT_DBG_RECTIFIED)
    bool resized = false;          // it resized (AMDAT_DBG_RESIZED)
    uint32_t raw = 0;              // it converted Bayer or 16-bit frames into d_raw with this instance (RAW_KIND_*; AMDAT_DBG_RAW_GRAY)
  } last;
  // quad_sigma (amdAprilTagsSetQuadSigma): the filter runs while qs_ksz > 1; qs.tk are the taps of the k_quad_sigma<qs_kh> instance
  uint32_t qs_ksz = 1;
  int qs_kh = 0;
  QsTaps qs = {};
  // amdAprilTagsSetPerFrameSizes: every frame of a submission brings its own size, up to the handle's (check_images, fill_frames)
  bool per_frame_sizes = false;
  // The front stage.  amdAprilTagsSetRectification: frame i of a submission is undistorted with rect_models[i % size] into slot i of
  // the front plane (d_conv: such a submission never takes the conversion launch) by k_rectify_frames, and the pipeline sees that slot
  // as a mono8 frame.  amdAprilTagsSetResize: frame i, at any source size, is resized to resize_sizes[i % size] into the same slot by
  // k_resize_frames -- through the rectification where that is on, in place of k_rectify_frames -- and detected there
  std::vector<amdAprilTagsCameraModelEx_t> rect_models; // empty: off (amdAprilTagsSetRectification stores plumb_bob, R = I)
  bool rect_general = false;                            // some model needs the general projection: the front launch is the _general kernel
  std::vector<amdAprilTagsSize_t> resize_sizes;         // empty: off
  HostBuf<FrontDesc> h_front;                           // pinned, one per batch slot: k_prologue uploads them with the frame descriptors
  DevBuf<FrontDesc> d_front;
  std::vector<amdAprilTagsImageInput_t> front_imgs;     // the plane's slots as the mono8 images of the submission (fill_front)
  // Raw formats (raw_formats.h): frame i of a Bayer or 16-bit submission is converted into slot i of d_raw by k_raw_to_mono8_frames, ahead
  // of the front stage, and the rest sees that slot as a mono8 frame.  The plane has max_batch slots at the largest source size seen so
  // far (with amdAprilTagsSetResize a source may exceed the handle's size); it is allocated by the first raw submission and regrown
  // before the enqueue when a larger source arrives.  Its pointers travel through the descriptor block: no captured graph carries them.
  DevBuf<uint8_t> d_raw;
  size_t raw_pitch = 0;                                 // a multiple of 64
  uint32_t raw_w = 0, raw_h = 0;                        // the slot's extent
  uint32_t raw_shift = RAW_MAX_SHIFT;                   // amdAprilTagsSetRawShift: host state that travels with the descriptors
  HostBuf<RawDesc> h_rawdesc;                           // pinned, one per batch slot
  DevBuf<RawDesc> d_rawdesc;
  std::vector<amdAprilTagsImageInput_t> raw_imgs;       // the plane's slots as the mono8 images of the submission (fill_raw)
  // What the post stages own, each set allocated by the first call that turns its stage on -- the layouts at their largest size,
  // the iteration count and sigma^2 in device memory -- so that a later value changes no launch argument.
  // amdAprilTagsSetBundles (bundle_layout.h):
  DevBuf<BundleHeadDev> d_bundle_head;
  DevBuf<BundleMemberDev> d_bundle_members;             // AMDAT_MAX_BUNDLE_MEMBERS
  DevBuf<uint16_t> d_bundle_table;                      // one entry per code of every family of the handle
  HostBuf<BundlePoseRec> h_bposes;                      // pinned, max_batch x AMDAT_MAX_BUNDLES: k_bundle_pose writes frame * nbundles + bundle
  // amdAprilTagsSetBundlesEx (rigid_layout.h):
  DevBuf<RigidHeadDev> d_rigid_head;
  DevBuf<RigidMemberDev> d_rigid_members;               // RIGID_MAX_MEMBERS
  DevBuf<uint16_t> d_rigid_table;                       // one entry per code of every family of the handle
  HostBuf<RigidPoseRec> h_xposes;                       // pinned, max_batch x AMDAT_MAX_BUNDLES: k_bundle_rigid writes frame * nrigid + bundle
  // amdAprilTagsSetPoseRefinement:
  DevBuf<uint32_t> d_pose_cfg;                          // [0]: the iteration count
  HostBuf<PoseRefineRec> h_rposes;                      // pinned, max_batch x dcap: k_pose_refine writes frame * ostride + record, as k_reconcile does
  // amdAprilTagsSetPoseCovariance:
  DevBuf<double> d_cov_cfg;                             // [0]: sigma^2
  HostBuf<PoseCovRec> h_rcovs;                          // pinned, max_batch x dcap, beside h_rposes
  HostBuf<PoseCovRec> h_xcovs;                          // pinned, max_batch x AMDAT_MAX_BUNDLES, beside h_xposes
  // amdAprilTagsSetCornerUndistortion: frame i of a submission takes undist_models[i % size]; the slot's camera travels through the
  // pinned block h_ucams, which k_prologue uploads with the frame descriptors
  std::vector<amdAprilTagsCameraModelEx_t> undist_models;   // post.nundist of them
  HostBuf<UndistortCam> h_ucams;                        // pinned, one per batch slot
  DevBuf<UndistortCam> d_ucams;
  DevBuf<DetRec> d_dets_u;                              // max_batch x dcap, laid out and indexed as d_dets
  HostBuf<UndistortRec> h_udets;                        // pinned, max_batch x dcap: frame * ostride + record, as k_reconcile writes h_out
  // amdAprilTagsSetRig / amdAprilTagsSetRigSlots: batch slot i of a submission is camera rig_slots[i].camera of group
  // rig_slots[i].group (beyond the list: camera i % nrig of group i / nrig); each slot's group, camera and extrinsics travel through
  // the pinned block h_rig, which k_prologue uploads with the frame descriptors
  std::vector<amdAprilTagsRigCamera_t> rig_cams;        // post.nrig of them
  std::vector<amdAprilTagsRigSlot_t> rig_slots;
  HostBuf<RigSlotDev> h_rig;                            // pinned, one per batch slot
  DevBuf<RigSlotDev> d_rig;
  HostBuf<RigPoseRec> h_gposes;                         // pinned, max_batch x AMDAT_MAX_BUNDLES: k_bundle_rig writes group * nrigid + bundle
  // amdAprilTagsSetTagTable (tag_table.h): header, keys and sizes in one buffer of TT_BYTES, allocated by the first call with
  // entries and freed by the call without; null: no table.  k_reconcile, k_undistort_records and k_pose_refine take the pointer
  // as an argument, so a captured graph holds whether a table exists and nothing of its contents.
  DevBuf<uint8_t> d_tag_table;
};

// ------------------------------------------------------------------------------------------------
// small kernels that live with the host code
// ------------------------------------------------------------------------------------------------
__global__ void k_debug_math(int op, uint32_t n, const double* a, const double* b, double* out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (op == 0) out[i] = __dsqrt_rn(a[i]);
  else if (op == 1) out[i] = a[i] / b[i];
  else if (op == 2) out[i] = (double)at_sqrtf_rn((float)a[i]);
  else if (op == 3) out[i] = (double)__fdiv_rn((float)a[i], (float)b[i]);
  else if (op == 5) out[i] = sqrt_u18((uint32_t)a[i]);     // integer arguments below 2^18
  else if (op == 6) out[i] = atan_s(a[i]);                 // the equidistant model's arctangent (camera_models.h)
  else out[i] = div_by(a[i], b[i], shared_recip(b[i]));   // the line fit's shared-reciprocal division
}

// colour -> mono8 (gray_bt601, common.h): four adjacent pixels of row blockIdx.y per thread, the body of both kernels below
template <int NCH, int RIDX, int BIDX>
__device__ __forceinline__ void to_mono8_row(const uint8_t* __restrict__ src, size_t spitch, uint8_t* __restrict__ dst, size_t dpitch,
                                             uint32_t w, uint32_t h) {
  const uint32_t x4 = (blockIdx.x * 256 + threadIdx.x) * 4;
  const uint32_t y = blockIdx.y;
  if (x4 >= w || y >= h) return;
  const uint8_t* s = src + (size_t)y * spitch + (size_t)x4 * NCH;
  uint8_t* d = dst + (size_t)y * dpitch + x4;
  for (uint32_t k = 0; k < 4 && x4 + k < w; k++) d[k] = (uint8_t)gray_bt601(s[k * NCH + RIDX], s[k * NCH + 1], s[k * NCH + BIDX]);
}

template <int NCH, int RIDX, int BIDX>
__global__ __launch_bounds__(256) void k_to_mono8(const uint8_t* __restrict__ src, size_t spitch, uint8_t* __restrict__ dst,
                                                  size_t dpitch, uint32_t w, uint32_t h) {
  to_mono8_row<NCH, RIDX, BIDX>(src, spitch, dst, dpitch, w, h);
}

// The same conversion for the frames of a colour submission that does not take the fused loader of k_threshold (decimate > 1,
// tile_size 8): source and destination of frame blockIdx.z come from its descriptor (src -> img), one launch per submission.
// (the grid is the handle's size; w x h is the frame's own)
template <int NCH, int RIDX, int BIDX>
__global__ __launch_bounds__(256) void k_to_mono8_frames(const FrameDesc* __restrict__ frames) {
  const FrameDesc fd = frames[blockIdx.z];
  to_mono8_row<NCH, RIDX, BIDX>(fd.src, fd.src_pitch, const_cast<uint8_t*>(fd.img), fd.pitch, (uint32_t)fd.W0, (uint32_t)fd.H0);
}

// quad_sigma's taps, computed on the host once per setting: ksz = (int)(4 |sigma|) made odd, h = ksz / 2,
// dk[i] = exp(-0.5 ((i - h) / s)^2) normalised by their sum in index order, k[i] = (uint8_t)(dk[i] * 255).  ksz <= 1 is the identity.
static uint32_t quad_sigma_taps(float sigma, uint8_t k[QS_MAX_KSZ]) {
  const float s = fabsf(sigma);
  int ksz = (int)(4.0f * s);
  if ((ksz & 1) == 0) ksz++;
  if (ksz <= 1) return 1;
  if (ksz > QS_MAX_KSZ) return 0;
  const int h = ksz / 2;
  double dk[QS_MAX_KSZ];
  double acc = 0;
  for (int i = 0; i < ksz; i++) {
    const double x = (i - h) / (double)s;
    dk[i] = exp(-0.5 * x * x);
    acc += dk[i];
  }
  for (int i = 0; i < ksz; i++) k[i] = (uint8_t)(dk[i] / acc * 255.0);
  return (uint32_t)ksz;
}

// bytes per pixel of an encoding
static inline uint32_t enc_channels(uint32_t fmt) {
  if (raw_is_raw(fmt)) return raw_bytes_per_sample(fmt);
  return fmt == AMDAT_ENC_MONO8 ? 1u : (fmt <= AMDAT_ENC_BGR8 ? 3u : 4u);
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int amdAprilTagsEncodingFromName(const char* name) {
  if (!name) return -1;
  // src/apriltag_node.cpp:76-82, then the raw formats under their names in sensor_msgs/image_encodings (raw_formats.h)
  static const char* const kNames[14] = {"mono8", "rgb8", "bgr8", "rgba8", "bgra8", "bayer_rggb8", "bayer_bggr8", "bayer_gbrg8", "bayer_grbg8",
                                         "mono16", "bayer_rggb16", "bayer_bggr16", "bayer_gbrg16", "bayer_grbg16"};
  static_assert(AMDAT_ENC_BAYER_RGGB8 == (int)RAW_ENC_FIRST && AMDAT_ENC_MONO16 == (int)RAW_ENC_MONO16 && AMDAT_ENC_BAYER_GRBG16 == (int)RAW_ENC_LAST, "raw_formats.h");
  for (int i = 0; i < 14; i++) if (!strcmp(name, kNames[i])) return i;
  return -1;
}

void amdAprilTagsDefaultConfig(amdAprilTagsConfig_t* cfg, uint32_t width, uint32_t height) {
  memset(cfg, 0, sizeof(*cfg));
  cfg->struct_size = (uint32_t)sizeof(*cfg);
  cfg->width = width;
  cfg->height = height;
  cfg->tile_size = 4;
  cfg->decimate = 1;
  cfg->num_families = 1;
  cfg->families[0] = AMDAT_TAG36H11;
  cfg->intrinsics = {1000.0f, 1000.0f, width / 2.0f, height / 2.0f};
  cfg->tag_size = 0.22f;
  cfg->max_batch = 1;
  cfg->refine_edges = 1;
  cfg->max_hamming = 2;
  cfg->decode_sharpening = 0.25f;
  cfg->device = -1;
  cfg->no_graph_replay = 0;
  cfg->no_stream_priorities = 0;
}

uint32_t amdAprilTagsConfigLayoutVersion(void) { return AMDAT_CONFIG_LAYOUT_VERSION; }

// a registered name must fit the slot's buffer whole (a truncated name could never be found again), and a code word must not
// carry bits above the family's width (it could never match, and the Hamming search would count the stray bits)
static bool family_args_ok(const char* name, uint32_t nbits, const uint64_t* codes, uint32_t ncodes) {
  if (strlen(name) >= sizeof(FamilyHost::name_buf)) return false;
  if (nbits < 64)
    for (uint32_t i = 0; i < ncodes; i++)
      if (codes[i] >> nbits) return false;
  return true;
}

int amdAprilTagsRegisterFamily(amdAprilTagsFamily slot, const char* name, uint32_t d, const uint64_t* codes, uint32_t ncodes) {
  std::call_once(g_fam_once, init_families);
  if (!is_registrable_slot((int)slot)) return AMDAT_INVALID_ARGUMENT;
  if (!name || !codes || ncodes == 0 || d < 3 || d > 7) return AMDAT_INVALID_ARGUMENT;
  if (!family_args_ok(name, d * d, codes, ncodes)) return AMDAT_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(g_fam_mutex);
  FamilyHost& f = g_families[slot];
  f.owned.assign(codes, codes + ncodes);
  strncpy(f.name_buf, name, sizeof(f.name_buf) - 1);
  f.name_buf[sizeof(f.name_buf) - 1] = 0;
  f.name = f.name_buf;
  family_set_classic(f, d);
  f.ncodes = ncodes;
  f.codes = f.owned.data();
  return AMDAT_SUCCESS;
}

int amdAprilTagsRegisterFamilyEx(amdAprilTagsFamily slot, const char* name, uint32_t nbits, const int8_t* bit_x, const int8_t* bit_y,
                                 uint32_t width_at_border, uint32_t total_width, int reversed_border, const uint64_t* codes,
                                 uint32_t ncodes) {
  std::call_once(g_fam_once, init_families);
  if (!is_registrable_slot((int)slot)) return AMDAT_INVALID_ARGUMENT;
  if (!name || !bit_x || !bit_y || !codes || ncodes == 0 || nbits == 0 || nbits > 64) return AMDAT_INVALID_ARGUMENT;
  if (!family_args_ok(name, nbits, codes, ncodes)) return AMDAT_INVALID_ARGUMENT;
  if (width_at_border < 3 || total_width < width_at_border || total_width > 12 || ((total_width - width_at_border) & 1u))
    return AMDAT_INVALID_ARGUMENT;
  // k_decode_wave holds the 8 x width_at_border border samples of the gray models in LDS arrays of 80 entries: a border square of at
  // most 10 cells, which is what a classic 8 x 8 family (64 bits, the widest word) needs
  if (width_at_border > 10) return AMDAT_INVALID_ARGUMENT;
  FamilyHost f;
  f.d = 0; f.nbits = nbits; f.width_at_border = width_at_border; f.total_width = total_width; f.reversed_border = reversed_border ? 1 : 0;
  const int min_coord = ((int)width_at_border - (int)total_width) / 2;
  for (uint32_t i = 0; i < nbits; i++) {
    if (bit_x[i] < min_coord || bit_x[i] >= min_coord + (int)total_width || bit_y[i] < min_coord || bit_y[i] >= min_coord + (int)total_width)
      return AMDAT_INVALID_ARGUMENT;
    f.bit_x[i] = bit_x[i]; f.bit_y[i] = bit_y[i];
  }
  if (!family_finish_layout(f)) return AMDAT_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(g_fam_mutex);
  FamilyHost& g = g_families[slot];
  g = f;
  g.owned.assign(codes, codes + ncodes);
  strncpy(g.name_buf, name, sizeof(g.name_buf) - 1);
  g.name_buf[sizeof(g.name_buf) - 1] = 0;
  g.name = g.name_buf;
  g.ncodes = ncodes;
  g.codes = g.owned.data();
  return AMDAT_SUCCESS;
}

int amdAprilTagsUnregisterFamily(amdAprilTagsFamily slot) {
  std::call_once(g_fam_once, init_families);
  if (!is_registrable_slot((int)slot)) return AMDAT_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(g_fam_mutex);
  FamilyHost& f = g_families[slot];
  f.codes = nullptr; f.ncodes = 0; f.name = nullptr; f.name_buf[0] = 0;
  f.owned.clear();
  return AMDAT_SUCCESS;
}

int amdAprilTagsFamilyInfo(amdAprilTagsFamily family, const char** name, uint32_t* d, uint32_t* ncodes, const uint64_t** codes) {
  std::call_once(g_fam_once, init_families);
  if ((int)family < 0 || family >= AMDAT_ENUM_SIZE) return AMDAT_UNSUPPORTED;
  std::lock_guard<std::mutex> lk(g_fam_mutex);   // (the pointers handed out stay valid until the slot is registered again)
  if (g_families[family].codes == nullptr) return AMDAT_UNSUPPORTED;
  if (name) *name = g_families[family].name;
  if (d) *d = g_families[family].d;
  if (ncodes) *ncodes = g_families[family].ncodes;
  if (codes) *codes = g_families[family].codes;
  return AMDAT_SUCCESS;
}

int amdAprilTagsFamilyFromName(const char* name) {
  std::call_once(g_fam_once, init_families);
  if (!name) return -1;
  // registered tables take precedence over a built-in of the same name
  static const int scan[AMDAT_ENUM_SIZE] = {AMDAT_CUSTOM0, AMDAT_CUSTOM1, AMDAT_CUSTOM2, AMDAT_CUSTOM3, AMDAT_CUSTOM4,
                                            AMDAT_TAG36H10, AMDAT_TAG36H11, AMDAT_TAG25H9, AMDAT_TAG16H5};
  std::lock_guard<std::mutex> lk(g_fam_mutex);
  for (int k = 0; k < AMDAT_ENUM_SIZE; k++) {
    const int i = scan[k];
    if (g_families[i].codes && g_families[i].name && !strcmp(g_families[i].name, name)) return i;
  }
  return -1;
}

const char* amdAprilTagsStageName(uint32_t stage) { return stage < AMDAT_NUM_STAGES ? kStageNames[stage] : ""; }

// Every device allocation of a handle goes through these two, and only they change device_bytes (amdAprilTagsGetDeviceBytes).  An
// empty buffer gets 16 bytes (a valid launch argument).  A failed allocation leaves nothing behind: no holder, no pending error.
static bool dev_alloc(amdAprilTagsDetector_st* D, DevAlloc& b, size_t bytes) {
  if (!bytes) bytes = 16;
  if (hipMalloc(&b.p, bytes) != hipSuccess) { b.p = nullptr; (void)hipGetLastError(); return false; }
  b.bytes = bytes;
  D->device_bytes += bytes;
  if (std::find(D->owned.begin(), D->owned.end(), &b) == D->owned.end()) D->owned.push_back(&b);
  return true;
}
static void dev_free(amdAprilTagsDetector_st* D, DevAlloc& b) {
  if (b.p) hipFree(b.p);
  D->device_bytes -= b.bytes;
  b = DevAlloc();
}
// Replaces b's buffer, the new one allocated before the old one is freed (b is untouched if that fails).
static bool dev_regrow(amdAprilTagsDetector_st* D, DevAlloc& b, size_t bytes) {
  DevAlloc old = b;
  b = DevAlloc();
  if (!dev_alloc(D, b, bytes)) { b = old; return false; }
  dev_free(D, old);
  return true;
}

// The same for pinned host memory the kernels read (descriptors) and write (records, counters + stamp) over the bus: COHERENT
// (fine-grained) mapped memory, stated rather than left to the runtime's default -- the host reads it right after a stream wait, not
// after a device-wide one -- and zeroed.  Not counted in device_bytes.  A failed allocation leaves nothing behind, as dev_alloc's.
static bool host_alloc(amdAprilTagsDetector_st* D, HostAlloc& b, size_t bytes) {
  if (hipHostMalloc(&b.p, bytes, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) { b.p = nullptr; (void)hipGetLastError(); return false; }
  memset(b.p, 0, bytes);
  D->host_owned.push_back(&b);
  return true;
}
// First-use allocation: what a mode needs is allocated by the first call that turns it on, and kept.
static bool ensure_dev(amdAprilTagsDetector_st* D, DevAlloc& b, size_t bytes) { return b.p || dev_alloc(D, b, bytes); }
static bool ensure_host(amdAprilTagsDetector_st* D, HostAlloc& b, size_t bytes) { return b.p || host_alloc(D, b, bytes); }

static void free_all(amdAprilTagsDetector_st* D) {
  for (auto& g : D->graphs) if (g.exec) hipGraphExecDestroy(g.exec);
  for (hipGraphExec_t e : D->retired_graphs) hipGraphExecDestroy(e);
  for (DevAlloc* b : D->owned) dev_free(D, *b);   // (d_counters and d_ptprof point into d_workctl's and d_fqprof's allocations)
  for (HostAlloc* b : D->host_owned) hipHostFree(b->p);
  for (auto& e : D->ev) if (e) hipEventDestroy(e);
  if (D->own_stream) hipStreamDestroy(D->own_stream);
  for (auto& a : D->aux_stream) if (a) hipStreamDestroy(a);
  if (D->ev_fork) hipEventDestroy(D->ev_fork);
  for (auto& e : D->ev_join) if (e) hipEventDestroy(e);
}

// The pair table is empty between submissions: k_cluster_select, its last reader, empties every slot it finds used (a few
// per cent of the table), so a submission starts without the two table-sized fills it used to open with (201 MB per 256
// frames; on a one-frame call two of five 4-5 us fill launches ahead of the first kernel).  The whole table is only
// written here: after (re)allocation, and after a submission that did not run to its end (tables_dirty).
static int clear_hash_tables(amdAprilTagsDetector_st* D) {
  const size_t B = D->cfg.max_batch;
  // (this runs at creation and when a capacity changes, never in a steady-state call.  On the handle's OWN stream, and a wait for
  // that stream only: a legacy-stream fill would fail -- here, in this thread -- whenever another host thread's handle on the
  // same device is capturing its launch graph at that moment, and a device-wide wait would stall that thread's streams.  Round 4
  // had tried this and taken it out again over a crash "inside the regrowth test" that round 6 traced to hipGraphExecDestroy.)
  if (hipMemsetAsync(D->d_hkeys, 0xFF, B * (size_t)D->P.hcap * 8, D->own_stream) != hipSuccess) return AMDAT_HIP_ERROR;
  if (hipMemsetAsync(D->d_hcnt, 0, B * (size_t)D->P.hcap * 4, D->own_stream) != hipSuccess) return AMDAT_HIP_ERROR;
  if (hipStreamSynchronize(D->own_stream) != hipSuccess) return AMDAT_HIP_ERROR;
  D->tables_dirty = false;
  return AMDAT_SUCCESS;
}

// The component-pair table of P.hcap slots per frame.
static int alloc_hash_buffers(amdAprilTagsDetector_st* D) {
  DetParams& P = D->P;
  const size_t B = D->cfg.max_batch;
  { uint32_t lg = 0; while ((1u << lg) < P.hcap) lg++; P.hshift = 64 - lg; }
  dev_free(D, D->d_hkeys); dev_free(D, D->d_hcnt); dev_free(D, D->d_hoff);
  if (!dev_alloc(D, D->d_hkeys, B * (size_t)P.hcap * 8) || !dev_alloc(D, D->d_hcnt, B * (size_t)P.hcap * 4) ||
      !dev_alloc(D, D->d_hoff, B * (size_t)P.hcap * 4))
    return AMDAT_OUT_OF_MEMORY;
  return clear_hash_tables(D);
}

// Buffers whose size follows the point capacity P.pcap: staging words, long staging records, points and the quad fit's work lists (their
// capacities are bounded by points / smallest cluster of the class).  Called at creation and again when the capacity grows.
static int alloc_point_buffers(amdAprilTagsDetector_st* D) {
  DetParams& P = D->P;
  const size_t B = D->cfg.max_batch;
  { const int rc = plan_work_layouts(D->fq, P.pcap, P.ccap, (uint32_t)B, &D->work_layout); if (rc) return rc; }
  const size_t off = D->work_layout.words;
  // Long staging records (kernels_cluster.h) only occur where a 64 x 16 tile has more than 2048 emissions -- above two per pixel --
  // or more than 255 component pairs; an eighth of the point capacity is room for them on ordinary content.  An overflow reports
  // like a point overflow (AMDAT_FLAG_POINTS_OVERFLOW); the host tells the two apart by the counters and grows the list by itself
  // -- a quarter, half, all of the point capacity (plan_growth, growth.h): two-level noise near the percolation threshold puts more
  // than a quarter of its points there (a fuzz case of round 6: such a frame used to keep its overflow flag at the largest point
  // capacity).  Tools builds that shrink the tile's list start with the whole capacity.
#ifndef AMDAT_LCAP_DIV
#define AMDAT_LCAP_DIV 8
#endif
  if (D->lcap_div == 0) D->lcap_div = AMDAT_LCAP_DIV;
  P.lcap = long_capacity(P.pcap, D->lcap_div);
  DevAlloc* bufs[5] = {&D->d_stage, &D->d_long, &D->d_pts, &D->d_work, &D->d_work2};
  const size_t bytes[5] = {B * (size_t)P.pcap * 4, B * (size_t)P.lcap * 16, B * (size_t)P.pcap * 4, off * 4,
                           (off - D->work_layout.all.off[D->fq.prefilter_class]) * 4};
  for (DevAlloc* b : bufs) dev_free(D, *b);
  for (int i = 0; i < 5; i++)
    if (!dev_alloc(D, *bufs[i], bytes[i])) return AMDAT_OUT_OF_MEMORY;
  return AMDAT_SUCCESS;
}

int amdCreateAprilTagsDetectorEx(amdAprilTagsHandle* handle, const amdAprilTagsConfig_t* cfg_in) {
  std::call_once(g_fam_once, init_families);
  if (!handle || !cfg_in) return AMDAT_INVALID_ARGUMENT;
  *handle = nullptr;
  // the caller's struct may be an older, shorter one (include/apriltag_amd.h: struct_size): only its own bytes are read, the
  // fields beyond them keep the defaults
  // layout 1 (round 5, the first with a size field) ended behind corner_convention; nothing shorter was ever published with a size
  constexpr uint32_t kMinConfig = (uint32_t)offsetof(amdAprilTagsConfig_t, no_graph_replay);
  if (cfg_in->struct_size < kMinConfig || cfg_in->struct_size > sizeof(amdAprilTagsConfig_t)) return AMDAT_INVALID_ARGUMENT;
  amdAprilTagsConfig_t cfg;
  amdAprilTagsDefaultConfig(&cfg, 0, 0);
  memcpy(&cfg, cfg_in, cfg_in->struct_size);
  cfg.struct_size = (uint32_t)sizeof(cfg);
  if (cfg.width == 0 || cfg.height == 0 || cfg.max_batch == 0 || cfg.decimate == 0) return AMDAT_INVALID_ARGUMENT;
  if (cfg.max_batch > 65535) return AMDAT_BATCH_TOO_LARGE;   // a work item carries the batch slot in at most 16 bits
  if (cfg.tile_size != 4 && cfg.tile_size != 8) return AMDAT_UNSUPPORTED;   // (the reference's default and twice it)
  if (cfg.decimate > 4) return AMDAT_UNSUPPORTED;     // the threshold loader is instantiated for 1..4
  if (cfg.max_hamming > 3) return AMDAT_INVALID_ARGUMENT;  // AprilRobotics' own limit for the code search
  if (cfg.corner_convention > AMDAT_CORNERS_ROTATED_180) return AMDAT_INVALID_ARGUMENT;
  if (cfg.num_families < 1 || cfg.num_families > AT_MAX_FAMILIES) return AMDAT_INVALID_ARGUMENT;
  // the family tables are copied under the registry's lock: a concurrent amdAprilTagsRegisterFamily[Ex] cannot swap a table
  // out from under the copy
  // (only for the copy: creation itself -- allocations, uploads, a device-wide wait -- runs without the registry's lock, so hosts
  // that create their per-GPU handles in parallel, or register families meanwhile, are not serialised behind it)
  struct FamilyCopy { FamilyHost layout; std::vector<uint64_t> codes; };
  std::vector<FamilyCopy> fams(cfg.num_families);
  {
    std::lock_guard<std::mutex> fam_lock(g_fam_mutex);
    for (uint32_t i = 0; i < cfg.num_families; i++) {
      if ((int)cfg.families[i] < 0 || cfg.families[i] >= AMDAT_ENUM_SIZE || !g_families[cfg.families[i]].codes)
        return AMDAT_UNSUPPORTED;
      const FamilyHost& g = g_families[cfg.families[i]];
      fams[i].codes.assign(g.codes, g.codes + g.ncodes);
      fams[i].layout = g;
      fams[i].layout.owned.clear(); fams[i].layout.codes = nullptr; fams[i].layout.name = nullptr;
    }
  }
  const int W = 1 + ((int)cfg.width - 1) / (int)cfg.decimate, H = 1 + ((int)cfg.height - 1) / (int)cfg.decimate;
  if (W / (int)cfg.tile_size < 1 || H / (int)cfg.tile_size < 1 || 2 * W + 1 >= (1 << 14) || 2 * H + 1 >= (1 << 14)) return AMDAT_UNSUPPORTED;

  auto* D = new (std::nothrow) amdAprilTagsDetector_st();
  if (!D) return AMDAT_OUT_OF_MEMORY;
  D->cfg = cfg;
  int caller_device = -1;
  if (hipGetDevice(&caller_device) != hipSuccess) { delete D; return AMDAT_HIP_ERROR; }
  D->device = cfg.device >= 0 ? cfg.device : caller_device;
  DeviceGuard guard(D->device);
  if (!guard.ok) { delete D; return AMDAT_HIP_ERROR; }
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, D->device) == hipSuccess && prop.multiProcessorCount > 0) D->num_cus = prop.multiProcessorCount;
  }

  // (first: every creation-time fill and copy below runs on it -- no legacy-stream call in this library, see clear_hash_tables)
  if (hipStreamCreateWithFlags(&D->own_stream, hipStreamNonBlocking) != hipSuccess) { delete D; return AMDAT_HIP_ERROR; }
  DetParams& P = D->P;
  memset(&P, 0, sizeof(P));
  P.W0 = (int)cfg.width; P.H0 = (int)cfg.height; P.W = W; P.H = H;
  P.WS = (W + 15) & ~15;
  P.decimate = (int)cfg.decimate;
  P.tile = (int)cfg.tile_size;
  P.tw = W / P.tile; P.th = H / P.tile;
  P.min_white_black_diff = 5;
  P.min_component_size = 25;
  P.min_cluster_points = 24;
  P.max_cluster_points = 3 * (2 * W + 2 * H);
  P.max_nmaxima = 10;
  // exactness bounds of the two-double moment sums (kernels_quad.h, split_term): W * x * x < 2^31, < 2^15 points
  P.split_moments = (W <= 2048 && H <= 2048 && P.max_cluster_points < 32768) ? 1 : 0;
  P.refine_edges = cfg.refine_edges ? 1 : 0;
  P.max_hamming = (int)cfg.max_hamming;
  P.nfam = (int)cfg.num_families;
  P.cos_critical_rad = (double)(float)0x1.f838b8c811c17p-1;   // cos(10 deg) as upstream's FLOAT parameter field holds it
  P.max_line_fit_mse = 10.0;
  P.decode_sharpening = (double)cfg.decode_sharpening;
  P.tag_size = (double)cfg.tag_size;
  int min_tag_width = 1000000;
  for (int i = 0; i < P.nfam; i++) {
    const FamilyHost& f = fams[i].layout;
    P.fam[i].d = f.d; P.fam[i].nbits = f.nbits; P.fam[i].width_at_border = f.width_at_border; P.fam[i].total_width = f.total_width;
    P.fam[i].reversed_border = f.reversed_border; P.fam[i].ncodes = f.ncodes;
    memcpy(P.fam[i].bit_x, f.bit_x, 64); memcpy(P.fam[i].bit_y, f.bit_y, 64); memcpy(P.fam[i].rot_src, f.rot_src, 64);
    if ((int)P.fam[i].width_at_border < min_tag_width) min_tag_width = (int)P.fam[i].width_at_border;
    if (f.reversed_border) P.reversed_border |= 1; else P.normal_border |= 1;
  }
  min_tag_width = (int)((float)min_tag_width / (float)P.decimate);
  if (min_tag_width < 3) min_tag_width = 3;
  P.min_tag_width = min_tag_width;
  const uint32_t npx = (uint32_t)W * (uint32_t)H;
  // Boundary points per frame: 2 per pixel covers every content the fuzzer produces (thin diagonal lines come
  // closest); frames that binarise completely (noise on every 4x4 tile) measure ~0.85 per pixel.
  // Default: 1 per pixel, and the handle GROWS the point buffers (up to the hard 2 per pixel) and repeats the submission
  // when a frame reports AMDAT_FLAG_POINTS_OVERFLOW -- results never depend on the capacity, memory follows the content
  // (15 GB instead of 27 GB for the 256-frame 1080p handle).  An explicit max_points is taken as given and never grown.
  D->grow.points = cfg.max_points == 0;
  D->grow.pcap_hard = 2u * npx;
  P.pcap = cfg.max_points ? cfg.max_points : npx;
  // Component-pair table: one slot per N/8 pixels is what no content overflowed; a sigma-2 1080p frame has ~4 000 pairs, so
  // the table starts at N/32 slots (1 MB instead of 4 MB per frame to clear, probe and scan) and, like the point buffers,
  // doubles when a frame reports AMDAT_FLAG_HASH_OVERFLOW or fills beyond a quarter (an explicit hash_slots is never grown).
  D->grow.hash = cfg.hash_slots == 0;
  D->grow.hcap_hard = cfg.hash_slots ? next_pow2(cfg.hash_slots) : next_pow2(npx / 8 > 4096 ? npx / 8 : 4096);
  if (D->grow.hcap_hard < 256) D->grow.hcap_hard = 256;
  P.hcap = cfg.hash_slots ? D->grow.hcap_hard : next_pow2(npx / 32 > 4096 ? npx / 32 : 4096);
  if (P.hcap > D->grow.hcap_hard) P.hcap = D->grow.hcap_hard;
  // A work item of the quad fit is one word: (frame << wshift) | cluster index.  The frame takes the bits the handle's frame count
  // needs, the index the rest (at most 24): 256 frames per submission leave room for 2^24 clusters per frame, 65 536 frames for
  // 65 536.  A frame has at most one cluster per used slot of the pair table, so min(2^wshift, hcap_hard) bounds the list; it starts
  // at 65 536 (a sigma-2 1080p frame has 4 000 clusters) and, like the point buffers, GROWS when a frame reports
  // AMDAT_FLAG_CLUSTERS_OVERFLOW -- an eight-megapixel checkerboard of six-pixel cells has 116 000 (plan_growth).  An explicit
  // max_clusters is taken as given (clamped to the bound) and never grown.
  {
    uint32_t fbits = 0;
    while ((1ull << fbits) < (uint64_t)cfg.max_batch) fbits++;
    // (max_batch <= 65 535 was checked above: fbits <= 16)
    P.wshift = 32u - fbits > 24u ? 24u : 32u - fbits;
  }
#ifndef AMDAT_CCAP0
#define AMDAT_CCAP0 65536u   // (tools builds start lower, so that ordinary content exercises the growth)
#endif
  D->grow.ccap_hard = D->grow.hcap_hard < (1u << P.wshift) ? D->grow.hcap_hard : (1u << P.wshift);
  D->grow.clusters = cfg.max_clusters == 0;
  P.ccap = cfg.max_clusters ? cfg.max_clusters : (D->grow.ccap_hard < AMDAT_CCAP0 ? D->grow.ccap_hard : AMDAT_CCAP0);
  if (P.ccap > D->grow.ccap_hard) P.ccap = D->grow.ccap_hard;
  P.qcap = cfg.max_quads ? cfg.max_quads : (P.ccap < 16384 ? P.ccap : 16384);
  D->grow.quads = cfg.max_quads == 0;   // (a two-megapixel checkerboard of two-pixel cells has 29 000 quads: the list doubles and the
                                        // submission is repeated, end_batch; an explicit max_quads reports AMDAT_FLAG_QUADS_OVERFLOW)
  P.dcap = cfg.max_detections ? cfg.max_detections : 1024;
  if (P.dcap > 65535) P.dcap = 65535;

  const size_t B = cfg.max_batch;
  D->fq = plan_classes(P.max_cluster_points, P.split_moments != 0, (unsigned)D->num_cus, (uint32_t)B);

  bool ok = true;
  auto alloc = [&](DevAlloc& b, size_t bytes) { if (ok) ok = dev_alloc(D, b, bytes); };
  if (P.decimate > 1) alloc(D->d_gray, B * (size_t)H * P.WS);
  alloc(D->d_thr, B * (size_t)H * P.WS);
  if (P.tile != 4) { alloc(D->d_tmin, B * (size_t)P.tw * P.th); alloc(D->d_tmax, B * (size_t)P.tw * P.th); }
  alloc(D->d_label, B * (size_t)npx * 4);
  alloc(D->d_csize, B * (size_t)npx * 4);
  // tile-local roots that go to the list touch their 64 x 64 tile's perimeter, and components are disjoint: at most
  // 252 (perimeter pixels) per tile
  P.rcap = (uint32_t)(((W + CC_T - 1) / CC_T) * ((H + CC_T - 1) / CC_T)) * (4u * CC_T - 4u);
  alloc(D->d_roots, B * (size_t)P.rcap * 4);
  alloc(D->d_perim, B * (size_t)cc_perim_layout(W, H).words * 4);
  if (ok) ok = alloc_hash_buffers(D) == AMDAT_SUCCESS;   // (before the point buffers: it decides the staging format)
  {   // per block (64 x 16 tile) of k_points: header and component-pair table for k_scatter
    const size_t tiles = (size_t)((W + PT_TW - 1) / PT_TW) * (size_t)((H + PT_TH - 1) / PT_TH);
    alloc(D->d_bhdr, B * tiles * sizeof(uint2));
    alloc(D->d_btab, B * tiles * PT_TB * sizeof(uint2));
  }
  alloc(D->d_clusters, B * (size_t)P.ccap * sizeof(ClusterRec));
  if (ok) { const int rc = alloc_point_buffers(D); if (rc == AMDAT_BATCH_TOO_LARGE) { free_all(D); delete D; return rc; } ok = rc == AMDAT_SUCCESS; }
  for (int k = 0; k < FQ_NCLS; k++) {
    const FqClassSpec& c = D->fq.cls[k];
    if (c.kernel != FQ_QUADS || !(class_sees_clusters(D->fq, k, false) || class_sees_clusters(D->fq, k, true))) continue;
    alloc(D->fq_scratch[k].d_lf, (size_t)c.grid * c.slot_cap * 48);
    // smoothed errors stay in registers up to FQ_SMOOTH_REGS_OF(threads) points per thread; larger clusters need a second array
    if (c.slot_cap > FQ_SMOOTH_REGS_OF(c.nt) * c.nt || c.slot_cap > c.sort_cap) alloc(D->fq_scratch[k].d_errs, (size_t)c.grid * c.slot_cap * 16);
  }
  if (D->fq.cls[FQ_NCLS - 1].slot_cap > D->fq.cls[FQ_NCLS - 1].sort_cap) {   // clusters beyond the LDS key array exist
    const FqClassSpec& c = D->fq.cls[FQ_NCLS - 1];
    alloc(D->d_keys_scr, (size_t)c.grid * c.slot_cap * 8);
  }
  alloc(D->d_quads, B * (size_t)P.qcap * sizeof(QuadRec));
  // every kept cluster can become a candidate (ccap); the list starts at the quad capacity and grows when a frame fills it
  P.cand_cap = P.qcap;
  alloc(D->d_cands, B * (size_t)P.cand_cap * sizeof(FitCand));
  alloc(D->d_dets, B * (size_t)P.dcap * sizeof(DetRec));
  alloc(D->d_order, B * (size_t)P.dcap * 2);
  // work-list control words and frame counters share one allocation, cleared by ONE fill per submission
  alloc(D->d_workctl, 32 * 4 + B * sizeof(FrameCounters));
  if (ok) D->d_counters = reinterpret_cast<FrameCounters*>(D->d_workctl + 32);
  alloc(D->d_frames, B * sizeof(FrameDesc));
  alloc(D->d_fqprof, (64 + 8) * 8);
  D->d_ptprof = D->d_fqprof + 64;   // k_points' phase counters follow the quad fit's
  for (int i = 0; ok && i < P.nfam; i++) {
    const std::vector<uint64_t>& codes = fams[i].codes;
    alloc(D->d_codes[i], codes.size() * 8);
    if (ok && (hipMemcpyAsync(D->d_codes[i], codes.data(), codes.size() * 8, hipMemcpyHostToDevice, D->own_stream) != hipSuccess ||
               hipStreamSynchronize(D->own_stream) != hipSuccess)) ok = false;   // (`fams` is pageable: waited for before it goes)
    P.fam[i].codes = D->d_codes[i];
  }
  ok = ok && host_alloc(D, D->h_frames, B * sizeof(FrameDesc)) && host_alloc(D, D->h_counters, B * sizeof(FrameCounters)) &&
       host_alloc(D, D->h_out, B * (size_t)P.dcap * sizeof(DetRec));
  for (auto& e : D->ev) if (ok && hipEventCreate(&e) != hipSuccess) ok = false;
  // Side streams.  The persistent grids of the fit's classes each hold the whole chip's wave slots, so which class's workgroups
  // are placed first decides who runs beside whom.  A handle sized for throughput (more than eight frames per submission) gets
  // PRIORITISED side streams -- greatest, default, least: the class with the longest chains goes on the first and is placed
  // first, the one-wave and small-cluster kernels fill what it leaves -- and never captures launch graphs: replaying a graph whose
  // branches were captured on prioritised streams costs 0.25 ms per launch on this runtime (one frame: 0.39 -> 0.65 ms).  A handle
  // of up to eight frames keeps plain side streams and graph replay.  (Both sets on one handle -- seven streams -- slowed every
  // stage: 17.6 -> 18.1 ms per 256 frames; the runtime multiplexes its streams onto a few hardware queues.)
  D->aux_prioritised = cfg.max_batch > 8 && !cfg.no_stream_priorities;
  {
    int lo = 0, hi = 0;   // (numerically hi <= lo: hi is the greatest priority)
    if (D->aux_prioritised && hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { D->aux_prioritised = false; (void)hipGetLastError(); }
    // (What the runtime does with the streams' hardware queues is sensitive to the ORDER in which plain and prioritised streams
    // come into being in a process -- measured on ROCm 7.0 / 7.2, bench.py's step and one- / eight-frame calls of a small handle,
    // tools/stream_order.py, tools/bench_variant.py:
    //   throughput-sized handle first, small handle after it      17.30 ms per 256 frames | 0.49 ms one frame, 1.32 ms eight
    //   small handle first (its four plain streams alive)         17.5                    | 0.38, 1.05
    //   four plain streams created and destroyed first            18.0 (every stage)      | 0.38, 1.05
    //   ... created and destroyed after the prioritised ones      17.5                    | 0.47, 1.34
    //   no priorities at all (cfg.no_stream_priorities)           17.7                    | 0.38, 1.05
    // rocprofv3's kernel trace shows the graph branches of a small handle created after a prioritised one on that handle's
    // hardware queues.  The library does not try to steer this: the first row is what a process with one throughput-sized handle
    // gets, a node's process -- one small handle -- never meets a prioritised stream, and a process that mixes both creates the
    // small handles first or sets no_stream_priorities: include/apriltag_amd.h, INTEGRATION.md.)
    for (int k = 0; k < FQ_NAUX; k++) {
      const int pr = k == 0 ? hi : (k == 1 ? (lo + hi) / 2 : lo);
      if (ok && (D->aux_prioritised ? hipStreamCreateWithPriority(&D->aux_stream[k], hipStreamNonBlocking, pr)
                                    : hipStreamCreateWithFlags(&D->aux_stream[k], hipStreamNonBlocking)) != hipSuccess) ok = false;
    }
    if (D->aux_prioritised) D->graph_max_frames = 0;
  }
  if (ok && hipEventCreateWithFlags(&D->ev_fork, hipEventDisableTiming) != hipSuccess) ok = false;
  for (auto& e : D->ev_join) if (ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) ok = false;
  // dynamic LDS beyond 64 KB has to be allowed per kernel (once per device; not allowed while a stream is being captured)
  if (ok) {
      const void* fns[10] = {reinterpret_cast<const void*>(k_fit_quads<512, false>), reinterpret_cast<const void*>(k_fit_quads<512, true>),
                            reinterpret_cast<const void*>(k_fit_quads<FQ_NT_BIG, false>), reinterpret_cast<const void*>(k_fit_quads<256, false>),
                            reinterpret_cast<const void*>(k_fit_quads<128, false>), reinterpret_cast<const void*>(k_fit_quads<64, false>),
                            reinterpret_cast<const void*>(k_fit_quads<FQ_NT_BIG, true>), reinterpret_cast<const void*>(k_fit_quads<256, true>),
                            reinterpret_cast<const void*>(k_fit_quads<128, true>), reinterpret_cast<const void*>(k_fit_quads<64, true>)};
      for (const void* fn : fns) if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 157000) != hipSuccess) ok = false;
  }
  if (ok && D->d_thr) {
    // the padding columns of the working images are read by vector loads; define them once
    if (hipMemsetAsync(D->d_thr, 127, B * (size_t)H * P.WS, D->own_stream) != hipSuccess) ok = false;
    if (ok && D->d_gray && hipMemsetAsync(D->d_gray, 0, B * (size_t)H * P.WS, D->own_stream) != hipSuccess) ok = false;
    if (ok && hipStreamSynchronize(D->own_stream) != hipSuccess) ok = false;
  }
  if (!ok) {
    free_all(D);
    delete D;
    return AMDAT_OUT_OF_MEMORY;
  }
  if (cfg.no_graph_replay) D->graph_max_frames = 0;
  *handle = D;
  return AMDAT_SUCCESS;
}

int amdCreateAprilTagsDetector(amdAprilTagsHandle* handle, uint32_t img_width, uint32_t img_height, uint32_t tile_size,
                               amdAprilTagsFamily tag_family, const amdAprilTagsCameraIntrinsics_t* cam, float tag_dim) {
  if (!cam) return AMDAT_INVALID_ARGUMENT;
  amdAprilTagsConfig_t cfg;
  amdAprilTagsDefaultConfig(&cfg, img_width, img_height);
  cfg.tile_size = tile_size;
  cfg.families[0] = tag_family;
  cfg.intrinsics = *cam;
  cfg.tag_size = tag_dim;
  return amdCreateAprilTagsDetectorEx(handle, &cfg);
}

int amdAprilTagsDestroy(amdAprilTagsHandle handle) {
  if (!handle) return AMDAT_INVALID_ARGUMENT;
  DeviceGuard guard(handle->device);
  if (handle->own_stream) (void)hipStreamSynchronize(handle->own_stream);
  for (auto& a : handle->aux_stream) if (a) (void)hipStreamSynchronize(a);
  (void)hipDeviceSynchronize();   // (a caller's stream may have carried the last submission; fails harmlessly under another thread's capture)
  (void)hipGetLastError();
  const bool had_graphs = !handle->retired_graphs.empty() || [&]() { for (auto& g : handle->graphs) if (g.exec) return true; return false; }();
  free_all(handle);
  // (hipGraphExecDestroy followed, with no device-wide wait in between, by the capture, instantiation and launch of another graph
  // is the sequence that crashes inside PyTorch's bundled HIP 7.0 runtime -- retire_graph below -- and the next graph may be
  // another handle's: one run of the regrowth stress loop in the GPU suite died that way, handle after handle in one process)
  if (had_graphs) { (void)hipDeviceSynchronize(); (void)hipGetLastError(); }
  delete handle;
  return AMDAT_SUCCESS;
}

int amdAprilTagsGetDeviceBytes(amdAprilTagsHandle handle, size_t* bytes) {
  if (!handle || !bytes) return AMDAT_INVALID_ARGUMENT;
  *bytes = handle->device_bytes;
  return AMDAT_SUCCESS;
}

int amdAprilTagsSetProfiling(amdAprilTagsHandle handle, int enable) {
  if (!handle) return AMDAT_INVALID_ARGUMENT;
  handle->profiling = enable != 0;
  handle->fq_counters = enable >= 2;
  return AMDAT_SUCCESS;
}

static void drop_graphs(amdAprilTagsDetector_st* D);   // (defined with the submission code below)
static int ensure_gray_plane(amdAprilTagsDetector_st* D);

int amdAprilTagsDebugSetSubmissionPath(amdAprilTagsHandle handle, int path) {
  if (!handle || path < AMDAT_PATH_AUTO || path > AMDAT_PATH_THROUGHPUT) return AMDAT_INVALID_ARGUMENT;
  if (handle->inflight.active) return AMDAT_INVALID_ARGUMENT;   // (a regrowth relaunch inside the wait must run the set the submit reported)
  if (path == handle->path_mode) return AMDAT_SUCCESS;
  DeviceGuard guard(handle->device);
  if (!guard.ok) return AMDAT_HIP_ERROR;
  drop_graphs(handle);   // captured under the other path
  handle->path_mode = path;
  return AMDAT_SUCCESS;
}

int amdAprilTagsSetQuadSigma(amdAprilTagsHandle handle, float quad_sigma) {
  if (!handle || !std::isfinite(quad_sigma) || handle->inflight.active) return AMDAT_INVALID_ARGUMENT;
  if (fabsf(quad_sigma) > 4.0f) return AMDAT_UNSUPPORTED;
  uint8_t k[QS_MAX_KSZ] = {};
  const uint32_t ksz = quad_sigma_taps(quad_sigma, k);
  QsTaps T = {};
  int kh = 0;
  if (ksz > 1) {
    const int h = (int)ksz / 2;
    kh = h <= 1 ? 1 : (h <= 2 ? 2 : (h <= 4 ? 4 : 8));
    for (int i = 0; i < (int)ksz; i++) T.tk[(i + kh - h) >> 2] |= (uint32_t)k[i] << (8 * ((i + kh - h) & 3));
    T.h = h;
    T.ksz = (int)ksz;
    T.sharpen = quad_sigma < 0.0f;
  }
  if (ksz == handle->qs_ksz && kh == handle->qs_kh && !memcmp(&T, &handle->qs, sizeof(T))) return AMDAT_SUCCESS;   // (identity -> identity)
  DeviceGuard guard(handle->device);
  if (!guard.ok) return AMDAT_HIP_ERROR;
  if (ksz > 1) { const int prc = ensure_gray_plane(handle); if (prc) return prc; }   // the filtered plane
  drop_graphs(handle);   // captured with the other filter state (the taps travel by value, the launch is there or not)
  handle->qs_ksz = ksz;
  handle->qs_kh = kh;
  handle->qs = T;
  return AMDAT_SUCCESS;
}

int amdAprilTagsSetPerFrameSizes(amdAprilTagsHandle handle, int enable) {
  if (!handle || handle->inflight.active) return AMDAT_INVALID_ARGUMENT;
  const bool on = enable != 0;
  if (on == handle->per_frame_sizes) return AMDAT_SUCCESS;
  DeviceGuard guard(handle->device);
  if (!guard.ok) return AMDAT_HIP_ERROR;
  drop_graphs(handle);   // captured with the other mode's launch set (the leftover kernel of the one-pass threshold: launch_threshold)
  handle->per_frame_sizes = on;
  return AMDAT_SUCCESS;
}

// The handle's full-size mono8 plane, max_batch slots at conv_pitch: the front plane of rectified and resized submissions, and the
// plane of colour submissions that take the conversion launch (no submission is both).
static int ensure_conv_plane(amdAprilTagsDetector_st* D) {
  if (D->d_conv) return AMDAT_SUCCESS;
  D->conv_pitch = ((size_t)D->cfg.width + 63) & ~(size_t)63;
  return dev_alloc(D, D->d_conv, D->cfg.max_batch * D->conv_pitch * D->cfg.height) ? AMDAT_SUCCESS : AMDAT_OUT_OF_MEMORY;
}
static uint8_t* conv_slot(const amdAprilTagsDetector_st* D, uint32_t i) { return D->d_conv + (size_t)i * D->conv_pitch * D->cfg.height; }

// What the first call that turns rectification or the resize on allocates: the front plane and the descriptor blocks of the front kernels.
static int ensure_front_buffers(amdAprilTagsDetector_st* D) {
  const size_t B = D->cfg.max_batch;
  { const int rc = ensure_conv_plane(D); if (rc) return rc; }
  if (!ensure_dev(D, D->d_front, B * sizeof(FrontDesc)) || !ensure_host(D, D->h_front, B * sizeof(FrontDesc))) return AMDAT_OUT_OF_MEMORY;
  D->front_imgs.resize(B);
  return AMDAT_SUCCESS;
}

// What amdAprilTagsSetRectificationEx and amdAprilTagsRectifyMono8Ex refuse in a camera model.
static bool camera_model_ok(const amdAprilTagsCameraModelEx_t& m) {
  static const int ncoef[3] = {5, 8, 4};   // plumb_bob, rational_polynomial, equidistant
  if (m.kind > AMDAT_DISTORTION_EQUIDISTANT) return false;
  for (double v : m.K) if (!std::isfinite(v)) return false;
  for (double v : m.D) if (!std::isfinite(v)) return false;
  for (double v : m.R) if (!std::isfinite(v)) return false;
  for (double v : m.Knew) if (!std::isfinite(v)) return false;
  if (m.Knew[0] == 0.0 || m.Knew[4] == 0.0) return false;
  for (int j = ncoef[m.kind]; j < 8; j++) if (m.D[j] != 0.0) return false;
  bool any = false;
  for (double v : m.R) any = any || v != 0.0;
  return any;   // (all zero: a CameraInfo that was never filled in)
}

// plumb_bob with R exactly the identity: the hoisted statement of section 7b serves it (one division a column)
static bool camera_model_general(const amdAprilTagsCameraModelEx_t& m) {
  if (m.kind != AMDAT_DISTORTION_PLUMB_BOB) return true;
  for (int j = 0; j < 9; j++) if (m.R[j] != (j % 4 == 0 ? 1.0 : 0.0)) return true;
  return false;
}

// The kernels' parameters of a camera model: D[0 .. 4] in RectifyParams' k1, k2, p1, p2, k3 for every kind (the equidistant
// projection reads its k1 .. k4 there), the rational denominator and the transpose of R (formed here, exactly) beside them.
static void camera_model_params(const amdAprilTagsCameraModelEx_t& m, RectifyParams& R, CamGeneral& G) {
  R = {m.K[0], m.K[4], m.K[2], m.K[5], m.D[0], m.D[1], m.D[2], m.D[3], m.D[4], m.Knew[0], m.Knew[4], m.Knew[2], m.Knew[5]};
  G.general = camera_model_general(m) ? 1u : 0u;
  G.kind = m.kind;
  G.k4 = m.D[5]; G.k5 = m.D[6]; G.k6 = m.D[7];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) G.Ri[3 * r + c] = m.R[3 * c + r];
}

int amdAprilTagsDistortionFromName(const char* name) {
  if (!name) return -1;
  if (!strcmp(name, "plumb_bob")) return AMDAT_DISTORTION_PLUMB_BOB;
  if (!strcmp(name, "rational_polynomial")) return AMDAT_DISTORTION_RATIONAL_POLYNOMIAL;
  if (!strcmp(name, "equidistant")) return AMDAT_DISTORTION_EQUIDISTANT;
  return -1;
}

int amdAprilTagsSetRectification(amdAprilTagsHandle handle, uint32_t ncams, const amdAprilTagsCameraModel_t* cams) {
  if (!handle || (ncams && !cams) || ncams > handle->cfg.max_batch) return AMDAT_INVALID_ARGUMENT;
  std::vector<amdAprilTagsCameraModelEx_t> ex(ncams);   // the Ex call with plumb_bob and R = I
  for (uint32_t c = 0; c < ncams; c++) {
    ex[c] = {};
    ex[c].kind = AMDAT_DISTORTION_PLUMB_BOB;
    memcpy(ex[c].K, cams[c].K, sizeof ex[c].K);
    memcpy(ex[c].D, cams[c].D, sizeof cams[c].D);
    memcpy(ex[c].Knew, cams[c].Knew, sizeof ex[c].Knew);
    ex[c].R[0] = ex[c].R[4] = ex[c].R[8] = 1.0;
  }
  return amdAprilTagsSetRectificationEx(handle, ncams, ncams ? ex.data() : nullptr);
}

int amdAprilTagsSetRectificationEx(amdAprilTagsHandle handle, uint32_t ncams, const amdAprilTagsCameraModelEx_t* cams) {
  if (!handle || handle->inflight.active || (ncams && !cams) || ncams > handle->cfg.max_batch) return AMDAT_INVALID_ARGUMENT;
  if (ncams && handle->post.nundist) return AMDAT_INVALID_ARGUMENT;   // (raw-frame mode is on: a frame is resampled or read raw, not both)
  bool general = false;
  for (uint32_t c = 0; c < ncams; c++) {
    if (!camera_model_ok(cams[c])) return AMDAT_INVALID_ARGUMENT;
    general = general || camera_model_general(cams[c]);
  }
  const bool on = ncams > 0;
  if (on != !handle->rect_models.empty()) {
    DeviceGuard guard(handle->device);
    if (!guard.ok) return AMDAT_HIP_ERROR;
    if (on) { const int rc = ensure_front_buffers(handle); if (rc) return rc; }
    drop_graphs(handle);   // captured with or without the rectification launch; the models themselves travel through the descriptors
  }
  handle->rect_models.assign(cams, cams + ncams);
  handle->rect_general = general;   // (which of the two front kernels a submission launches: a launch parameter, like the models no graph's concern -- see enqueue_submission)
  return AMDAT_SUCCESS;
}

int amdAprilTagsSetResize(amdAprilTagsHandle handle, uint32_t nsizes, const amdAprilTagsSize_t* sizes) {
  if (!handle || handle->inflight.active || (nsizes && !sizes) || nsizes > handle->cfg.max_batch) return AMDAT_INVALID_ARGUMENT;
  for (uint32_t c = 0; c < nsizes; c++)
    if (sizes[c].width == 0 || sizes[c].height == 0 || sizes[c].width > handle->cfg.width || sizes[c].height > handle->cfg.height)
      return AMDAT_INVALID_ARGUMENT;
  const bool on = nsizes > 0;
  if (on != !handle->resize_sizes.empty()) {
    DeviceGuard guard(handle->device);
    if (!guard.ok) return AMDAT_HIP_ERROR;
    if (on) { const int rc = ensure_front_buffers(handle); if (rc) return rc; }
    drop_graphs(handle);   // captured with or without the resize launch; the sizes themselves travel through the descriptors
  }
  handle->resize_sizes.assign(sizes, sizes + nsizes);
  return AMDAT_SUCCESS;
}

// ---- the stages behind k_reconcile (post_plan.h) -----------------------------------------------------------------------------
static_assert(POST_UD_WAVES == UD_WAVES_PER_FRAME && POST_PR_RECORDS_PER_WAVE == PR_RECORDS_PER_WAVE, "post_plan.h states the kernels' grids");

// Takes a setter's request into the mode.  The graphs are retired if and only if the request changes a stage's on / off bit: they
// were captured with or without each launch, and with the one or the other instance and record list.
static void set_post_mode(amdAprilTagsDetector_st* D, PostSetting what, double value) {
  const PostMode next = post_apply(D->post, what, value);
  if (post_graph_key(next) != post_graph_key(D->post)) drop_graphs(D);
  D->post = next;
}

// The planar and the rigid bundle setter.  Where it turns its kind on, the first call allocates the device layout at its largest
// size and the pinned record block; every such call uploads head, members and table and waits.
extern "C++" {   // (a template, inside the C ABI block)
template <class Layout, class Bundle, class Head, class Member, class Rec>
static int set_bundle_layout(amdAprilTagsDetector_st* D, PostSetting kind, uint32_t nbundles, const Bundle* bundles,
                             int (*build)(uint32_t, const uint32_t*, uint32_t, const Bundle*, Layout*), DevBuf<Head>& d_head,
                             DevBuf<Member>& d_members, size_t max_members, DevBuf<uint16_t>& d_table, HostBuf<Rec>& h_poses) {
  uint32_t ncodes[AT_MAX_FAMILIES] = {};
  for (int i = 0; i < D->P.nfam; i++) ncodes[i] = D->P.fam[i].ncodes;
  Layout L;
  { const int rc = build((uint32_t)D->P.nfam, ncodes, nbundles, bundles, &L); if (rc) return rc; }
  DeviceGuard guard(D->device);
  if (!guard.ok) return AMDAT_HIP_ERROR;
  if (nbundles > 0) {
    if (!ensure_dev(D, d_head, sizeof(Head)) || !ensure_dev(D, d_members, max_members * sizeof(Member)) ||
        !ensure_dev(D, d_table, L.table.size() * sizeof(uint16_t)) ||
        !ensure_host(D, h_poses, (size_t)D->cfg.max_batch * AMDAT_MAX_BUNDLES * sizeof(Rec)))
      return AMDAT_OUT_OF_MEMORY;
    // (no submission is in flight: nothing reads the layout; `L` is pageable, so the copies are waited for before it goes)
    const hipStream_t s = D->own_stream;
    HIP_TRY(hipMemcpyAsync(d_head, &L.head, sizeof(L.head), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_members, L.members.data(), L.members.size() * sizeof(Member), hipMemcpyHostToDevice, s));
    if (!L.table.empty()) HIP_TRY(hipMemcpyAsync(d_table, L.table.data(), L.table.size() * sizeof(uint16_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  set_post_mode(D, kind, nbundles);
  return AMDAT_SUCCESS;
}
}  // extern "C++"

int amdAprilTagsSetBundles(amdAprilTagsHandle handle, uint32_t nbundles, const amdAprilTagsBundle_t* bundles) {
  if (!handle || handle->inflight.active) return AMDAT_INVALID_ARGUMENT;
  return set_bundle_layout(handle, POST_SET_PLANAR, nbundles, bundles, bundle_layout_build, handle->d_bundle_head, handle->d_bundle_members,
                           AMDAT_MAX_BUNDLE_MEMBERS, handle->d_bundle_table, handle->h_bposes);
}

int amdAprilTagsSetBundlesEx(amdAprilTagsHandle handle, uint32_t nbundles, const amdAprilTagsBundleEx_t* bundles) {
  if (!handle || handle->inflight.active) return AMDAT_INVALID_ARGUMENT;
  static_assert(AMDAT_MAX_RIGID_BUNDLE_MEMBERS == RG_SLOTS, "the header's bound is the kernel's: one lane holds one tag");
  return set_bundle_layout(handle, POST_SET_RIGID, nbundles, bundles, rigid_layout_build, handle->d_rigid_head, handle->d_rigid_members,
                           RIGID_MAX_MEMBERS, handle->d_rigid_table, handle->h_xposes);
}

// The kernel's parameters of a camera model (undistort.h): K, D, R and Knew as they are given.
static UndistortCam undistort_cam(const amdAprilTagsCameraModelEx_t& m) {
  UndistortCam c = {};
  c.kind = m.kind;
  c.fx = m.K[0]; c.fy = m.K[4]; c.cx = m.K[2]; c.cy = m.K[5];
  for (int j = 0; j < 8; j++) c.d[j] = m.D[j];
  for (int j = 0; j < 9; j++) c.R[j] = m.R[j];
  c.nfx = m.Knew[0]; c.nfy = m.Knew[4]; c.ncx = m.Knew[2]; c.ncy = m.Knew[5];
  return c;
}

// What the first call that turns the corner undistortion on (or amdAprilTagsDebugUndistort) allocates.
static int ensure_undistort_buffers(amdAprilTagsDetector_st* D) {
  const size_t B = D->cfg.max_batch;
  static_assert(sizeof(UndistortCam) % 4 == 0, "k_prologue copies words");
  return ensure_host(D, D->h_ucams, B * sizeof(UndistortCam)) && ensure_dev(D, D->d_ucams, B * sizeof(UndistortCam)) &&
         ensure_dev(D, D->d_dets_u, B * (size_t)D->P.dcap * sizeof(DetRec)) &&
         ensure_host(D, D->h_udets, B * (size_t)D->P.dcap * sizeof(UndistortRec)) ? AMDAT_SUCCESS : AMDAT_OUT_OF_MEMORY;
}

int amdAprilTagsSetCornerUndistortion(amdAprilTagsHandle handle, uint32_t ncams, const amdAprilTagsCameraModelEx_t* cams) {
  if (!handle || handle->inflight.active || (ncams && !cams) || ncams > handle->cfg.max_batch) return AMDAT_INVALID_ARGUMENT;
  if (ncams && !handle->rect_models.empty()) return AMDAT_INVALID_ARGUMENT;   // (rectification is on: a frame is resampled or read raw, not both)
  for (uint32_t c = 0; c < ncams; c++)
    if (!camera_model_ok(cams[c])) return AMDAT_INVALID_ARGUMENT;
  const bool on = ncams > 0;
  if (on != (handle->post.nundist > 0)) {
    DeviceGuard guard(handle->device);
    if (!guard.ok) return AMDAT_HIP_ERROR;
    if (on) { const int rc = ensure_undistort_buffers(handle); if (rc) return rc; }
  }
  set_post_mode(handle, POST_SET_UNDISTORT, ncams);   // (the models travel through the descriptors)
  handle->undist_models.assign(cams, cams + ncams);
  return AMDAT_SUCCESS;
}

// One value of a mode that lives in device memory.  (No submission is in flight: nothing reads it; the source is pageable, so the
// copy is waited for before it goes.)
static int upload_value(amdAprilTagsDetector_st* D, void* dst, const void* value, size_t bytes) {
  HIP_TRY(hipMemcpyAsync(dst, value, bytes, hipMemcpyHostToDevice, D->own_stream));
  HIP_TRY(hipStreamSynchronize(D->own_stream));
  return AMDAT_SUCCESS;
}

int amdAprilTagsSetPoseRefinement(amdAprilTagsHandle handle, uint32_t iterations) {
  if (!handle || iterations > AMDAT_MAX_POSE_ITERATIONS || handle->inflight.active) return AMDAT_INVALID_ARGUMENT;
  static_assert(AMDAT_MAX_POSE_ITERATIONS == PR_MAX_ITERATIONS, "the header's bound is the kernel's");
  if (iterations > 0) {
    DeviceGuard guard(handle->device);
    if (!guard.ok) return AMDAT_HIP_ERROR;
    if (!ensure_dev(handle, handle->d_pose_cfg, 64) ||
        !ensure_host(handle, handle->h_rposes, (size_t)handle->cfg.max_batch * handle->P.dcap * sizeof(PoseRefineRec)))
      return AMDAT_OUT_OF_MEMORY;
    const int rc = upload_value(handle, handle->d_pose_cfg, &iterations, sizeof(iterations));
    if (rc) return rc;
  }
  set_post_mode(handle, POST_SET_REFINE, iterations);
  return AMDAT_SUCCESS;
}

int amdAprilTagsSetPoseCovariance(amdAprilTagsHandle handle, double corner_sigma_px) {
  if (!handle || !std::isfinite(corner_sigma_px) || corner_sigma_px < 0.0 || handle->inflight.active) return AMDAT_INVALID_ARGUMENT;
  if (corner_sigma_px > 0.0) {
    DeviceGuard guard(handle->device);
    if (!guard.ok) return AMDAT_HIP_ERROR;
    if (!ensure_dev(handle, handle->d_cov_cfg, 64) ||
        !ensure_host(handle, handle->h_rcovs, (size_t)handle->cfg.max_batch * handle->P.dcap * sizeof(PoseCovRec)) ||
        !ensure_host(handle, handle->h_xcovs, (size_t)handle->cfg.max_batch * AMDAT_MAX_BUNDLES * sizeof(PoseCovRec)))
      return AMDAT_OUT_OF_MEMORY;
    const double sigma2 = corner_sigma_px * corner_sigma_px;
    const int rc = upload_value(handle, handle->d_cov_cfg, &sigma2, sizeof(sigma2));
    if (rc) return rc;
  }
  set_post_mode(handle, POST_SET_COV, corner_sigma_px);
  return AMDAT_SUCCESS;
}

// The tag table (tag_table.h).  Built and checked on the host first: a refused call has touched nothing.  The contents go into the
// handle's buffer, which no launch reads now (no submission is in flight); only a table where there was none, or none where there
// was one, changes a launch argument and retires the graphs.
int amdAprilTagsSetTagTable(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsTagEntry_t* entries, uint32_t listed_only) {
  if (!handle || handle->inflight.active || (n && !entries) || n > AMDAT_MAX_TAG_ENTRIES || listed_only > 1u) return AMDAT_INVALID_ARGUMENT;
  amdAprilTagsDetector_st* D = handle;
  std::vector<uint8_t> image(TT_BYTES, 0);
  if (n) {
    uint32_t ncodes[AT_MAX_FAMILIES] = {};
    static_assert(AT_MAX_FAMILIES == TT_MAX_FAMILIES, "tag_table.h: a family index takes two bits of the key");
    for (int i = 0; i < D->P.nfam; i++) ncodes[i] = D->P.fam[i].ncodes;
    std::vector<TagTableEntry> list(n);
    for (uint32_t i = 0; i < n; i++) {
      if (entries[i].reserved) return AMDAT_INVALID_ARGUMENT;
      list[i] = {entries[i].family_index, entries[i].id, entries[i].size};
    }
    TagTableHeader head = {n, listed_only, {0u, 0u}};
    memcpy(image.data(), &head, sizeof(head));
    static_assert(sizeof(TagTableHeader) == TT_KEYS_OFFSET && TT_SIZES_OFFSET % 8 == 0, "tag_table.h: the buffer's layout");
    if (tt_build((uint32_t)D->P.nfam, ncodes, n, list.data(), reinterpret_cast<uint32_t*>(image.data() + TT_KEYS_OFFSET),
                 reinterpret_cast<double*>(image.data() + TT_SIZES_OFFSET)))
      return AMDAT_INVALID_ARGUMENT;
  }
  DeviceGuard guard(D->device);
  if (!guard.ok) return AMDAT_HIP_ERROR;
  const bool had = D->d_tag_table.p != nullptr;
  if (n) {
    if (!ensure_dev(D, D->d_tag_table, TT_BYTES)) return AMDAT_OUT_OF_MEMORY;
    const int rc = upload_value(D, D->d_tag_table.p, image.data(), TT_BYTES);
    if (rc) { if (!had) dev_free(D, D->d_tag_table); return rc; }
  } else if (had) {
    HIP_TRY(hipStreamSynchronize(D->own_stream));
    dev_free(D, D->d_tag_table);
  }
  if (had != (n > 0)) drop_graphs(D);
  return AMDAT_SUCCESS;
}

// The camera rig.  The first call that turns it on allocates the slot descriptors and the pinned record block; the extrinsics and
// the slot map are host state that fill_rig writes into every submission's descriptors.
int amdAprilTagsSetRig(amdAprilTagsHandle handle, uint32_t ncams, const amdAprilTagsRigCamera_t* cams) {
  if (!handle || handle->inflight.active || (ncams && !cams) || ncams > AMDAT_MAX_RIG_CAMERAS) return AMDAT_INVALID_ARGUMENT;
  static_assert(AMDAT_MAX_RIG_OBSERVATIONS == RG_SLOTS, "the header's bound is the kernel's: one lane holds one observation");
  for (uint32_t c = 0; c < ncams; c++) {
    for (int e = 0; e < 9; e++) if (!std::isfinite(cams[c].R[e])) return AMDAT_INVALID_ARGUMENT;
    for (int e = 0; e < 3; e++) if (!std::isfinite(cams[c].t[e])) return AMDAT_INVALID_ARGUMENT;
    if (!rigid_is_rotation(cams[c].R)) return AMDAT_INVALID_ARGUMENT;
  }
  if (ncams > 0) {
    DeviceGuard guard(handle->device);
    if (!guard.ok) return AMDAT_HIP_ERROR;
    const size_t B = handle->cfg.max_batch;
    static_assert(sizeof(RigSlotDev) % 4 == 0, "k_prologue copies words");
    if (!ensure_host(handle, handle->h_rig, B * sizeof(RigSlotDev)) || !ensure_dev(handle, handle->d_rig, B * sizeof(RigSlotDev)) ||
        !ensure_host(handle, handle->h_gposes, B * AMDAT_MAX_BUNDLES * sizeof(RigPoseRec)))
      return AMDAT_OUT_OF_MEMORY;
  }
  set_post_mode(handle, POST_SET_RIG, ncams);   // (the extrinsics travel through the descriptors)
  handle->rig_cams.assign(cams, cams + ncams);
  return AMDAT_SUCCESS;
}

int amdAprilTagsSetRigSlots(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsRigSlot_t* slots) {
  if (!handle || handle->inflight.active || (n && !slots) || n > handle->cfg.max_batch) return AMDAT_INVALID_ARGUMENT;
  handle->rig_slots.assign(slots, slots + n);
  return AMDAT_SUCCESS;
}

// The rig descriptors of a submission of n frames: each slot's group, camera and extrinsics.  AMDAT_INVALID_ARGUMENT, with nothing
// enqueued: a group index at or above n, a camera index at or above the rig's count, one (group, camera) named by two slots.
static int fill_rig(amdAprilTagsDetector_st* D, uint32_t n) {
  const uint32_t ncams = D->post.nrig;
  for (uint32_t i = 0; i < n; i++) {
    amdAprilTagsRigSlot_t sl = {i / ncams, i % ncams};
    if (i < D->rig_slots.size()) sl = D->rig_slots[i];
    RigSlotDev& r = D->h_rig[i];
    memset(&r, 0, sizeof(r));
    r.group = sl.group; r.camera = sl.camera;
    if (sl.camera == AMDAT_RIG_NO_CAMERA) continue;
    if (sl.group >= n || sl.camera >= ncams) return AMDAT_INVALID_ARGUMENT;
    for (uint32_t j = 0; j < i; j++)
      if (D->h_rig[j].camera == sl.camera && D->h_rig[j].group == sl.group) return AMDAT_INVALID_ARGUMENT;
    for (int e = 0; e < 9; e++) r.R[e] = D->rig_cams[sl.camera].R[e];
    for (int e = 0; e < 3; e++) r.t[e] = D->rig_cams[sl.camera].t[e];
  }
  return AMDAT_SUCCESS;
}

// Record i of `frame` of the last submission was refined from an invalid undistorted twin.
static bool undistorted_invalid(const amdAprilTagsDetector_st* D, uint32_t frame, uint32_t i) {
  return D->last.post.nundist && D->h_udets[(size_t)frame * D->last.ostride + i].det.status != AMDAT_UNDISTORT_OK;
}

// The per-frame getters: `field` of the first min(nout, ostride) records of `frame` in a block laid out as k_reconcile's, where
// the last submission ran the stages `stages` (post_graph_key bits).  `invalid` rewrites what comes of an invalid twin (section 7h:
// nothing of it is handed out).
extern "C++" {   // (templates, inside the C ABI block)
template <class Rec, class Out, class Invalid>
static int get_frame_records(amdAprilTagsDetector_st* D, uint32_t stages, const HostBuf<Rec>& block, Out Rec::*field, uint32_t frame,
                             Out* out, uint32_t capacity, uint32_t* n, Invalid invalid) {
  if (!out || !n || D->inflight.active || (post_graph_key(D->last.post) & stages) != stages || frame >= D->last.n) return AMDAT_INVALID_ARGUMENT;
  uint32_t k = D->h_counters[frame].nout;
  if (k > D->last.ostride) k = D->last.ostride;
  *n = k;
  if (capacity < k) return AMDAT_INVALID_ARGUMENT;
  const Rec* const recs = block + (size_t)frame * D->last.ostride;
  for (uint32_t i = 0; i < k; i++) {
    out[i] = recs[i].*field;
    if (undistorted_invalid(D, frame, i)) invalid(out[i]);
  }
  return AMDAT_SUCCESS;
}
// The per-bundle getters: `field` of nframes x bundles records, bundles being the last submission's count of the one kind.
template <class Rec, class Out>
static int get_bundle_records(amdAprilTagsDetector_st* D, uint32_t stages, uint32_t PostMode::*count, const HostBuf<Rec>& block,
                              Out Rec::*field, Out* out, uint32_t nframes) {
  if (!out || D->inflight.active || (post_graph_key(D->last.post) & stages) != stages || nframes > D->last.n) return AMDAT_INVALID_ARGUMENT;
  const size_t n = (size_t)nframes * D->last.post.*count;
  for (size_t i = 0; i < n; i++) out[i] = block[i].*field;
  return AMDAT_SUCCESS;
}
}  // extern "C++"

int amdAprilTagsGetBundlePoses(amdAprilTagsHandle handle, amdAprilTagsBundlePose_t* out, uint32_t nframes) {
  if (!handle) return AMDAT_INVALID_ARGUMENT;
  return get_bundle_records(handle, POST_PLANAR, &PostMode::nbundles, handle->h_bposes, &BundlePoseRec::pose, out, nframes);
}

int amdAprilTagsGetBundlePosesEx(amdAprilTagsHandle handle, amdAprilTagsBundlePoseEx_t* out, uint32_t nframes) {
  if (!handle) return AMDAT_INVALID_ARGUMENT;
  return get_bundle_records(handle, POST_RIGID, &PostMode::nrigid, handle->h_xposes, &RigidPoseRec::pose, out, nframes);
}

int amdAprilTagsGetBundlePoseCovariancesEx(amdAprilTagsHandle handle, amdAprilTagsPoseCovariance_t* out, uint32_t nframes) {
  if (!handle) return AMDAT_INVALID_ARGUMENT;
  return get_bundle_records(handle, POST_RIGID | POST_COV, &PostMode::nrigid, handle->h_xcovs, &PoseCovRec::c, out, nframes);
}

// (ngroups x bundles: a group index per frame of the submission, every entry written)
int amdAprilTagsGetRigBundlePoses(amdAprilTagsHandle handle, amdAprilTagsRigBundlePose_t* out, uint32_t ngroups) {
  if (!handle) return AMDAT_INVALID_ARGUMENT;
  return get_bundle_records(handle, POST_RIGID | POST_RIG, &PostMode::nrigid, handle->h_gposes, &RigPoseRec::pose, out, ngroups);
}

int amdAprilTagsGetUndistortedDetections(amdAprilTagsHandle handle, uint32_t frame, amdAprilTagsUndistortedDetection_t* out, uint32_t capacity, uint32_t* n) {
  if (!handle) return AMDAT_INVALID_ARGUMENT;
  return get_frame_records(handle, POST_UNDISTORT, handle->h_udets, &UndistortRec::det, frame, out, capacity, n,
                           [](amdAprilTagsUndistortedDetection_t&) {});   // (an invalid twin says so itself)
}

int amdAprilTagsGetRefinedPoses(amdAprilTagsHandle handle, uint32_t frame, amdAprilTagsRefinedPose_t* out, uint32_t capacity, uint32_t* n) {
  if (!handle) return AMDAT_INVALID_ARGUMENT;
  return get_frame_records(handle, POST_REFINE, handle->h_rposes, &PoseRefineRec::pose, frame, out, capacity, n,
                           [](amdAprilTagsRefinedPose_t& o) { o = {}; o.status = AMDAT_POSE_DEGENERATE; });
}

int amdAprilTagsGetRefinedPoseCovariances(amdAprilTagsHandle handle, uint32_t frame, amdAprilTagsPoseCovariance_t* out, uint32_t capacity, uint32_t* n) {
  if (!handle) return AMDAT_INVALID_ARGUMENT;
  return get_frame_records(handle, POST_REFINE | POST_COV, handle->h_rcovs, &PoseCovRec::c, frame, out, capacity, n,
                           [](amdAprilTagsPoseCovariance_t& o) { o = {}; });   // (all zero, valid = 0)
}

int amdAprilTagsDebugQuadSigmaTaps(float quad_sigma, uint8_t* taps, uint32_t capacity, uint32_t* ksz) {
  if (!ksz || !std::isfinite(quad_sigma)) return AMDAT_INVALID_ARGUMENT;
  if (fabsf(quad_sigma) > 4.0f) return AMDAT_UNSUPPORTED;
  uint8_t k[QS_MAX_KSZ] = {};
  *ksz = quad_sigma_taps(quad_sigma, k);
  if (*ksz > 1) {
    if (!taps || capacity < *ksz) return AMDAT_INVALID_ARGUMENT;
    memcpy(taps, k, *ksz);
  }
  return AMDAT_SUCCESS;
}

int amdAprilTagsDebugLateWaits(amdAprilTagsHandle handle) { return handle ? (int)handle->late_waits : -1; }

int amdAprilTagsDebugGraphReplay(amdAprilTagsHandle handle, uint32_t* live_graphs, uint32_t* retired_graphs) {
  if (!handle) return -1;
  uint32_t live = 0;
  for (const auto& g : handle->graphs) live += g.exec ? 1u : 0u;
  if (live_graphs) *live_graphs = live;
  if (retired_graphs) *retired_graphs = (uint32_t)handle->retired_graphs.size();
  return handle->graph_max_frames ? 1 : 0;
}

int amdAprilTagsDebugLastGraphNodes(amdAprilTagsHandle handle) { return handle ? (int)handle->last_graph_nodes : -1; }

int amdAprilTagsDebugLastSubmissionPath(amdAprilTagsHandle handle) {
  return handle ? handle->last_path : -1;
}

int amdAprilTagsGetStageMs(amdAprilTagsHandle handle, float* ms) {
  if (!handle || !ms) return AMDAT_INVALID_ARGUMENT;
  memcpy(ms, handle->stage_ms, sizeof(handle->stage_ms));
  return AMDAT_SUCCESS;
}

// resizing: the submission resizes (every submitting call with amdAprilTagsSetResize on; ThresholdOnly never).  The size the frame is
// detected at -- its target size then, its own otherwise -- obeys the size rules; the source size of a resized frame is free.
static int check_images(amdAprilTagsDetector_st* D, uint32_t n, const amdAprilTagsImageInput_t* images, uint32_t fmt = AMDAT_ENC_MONO8,
                        bool resizing = false) {
  if (n == 0 || !images) return AMDAT_INVALID_ARGUMENT;
  if (fmt > AMDAT_ENC_BAYER_GRBG16) return AMDAT_UNSUPPORTED;
  if (n > D->cfg.max_batch) return AMDAT_BATCH_TOO_LARGE;
  const uint32_t nsizes = (uint32_t)D->resize_sizes.size();
  for (uint32_t i = 0; i < n; i++) {
    if (!images[i].dev_ptr) return AMDAT_INVALID_ARGUMENT;
    uint32_t fw = images[i].width, fh = images[i].height;
    if (resizing) {
      if (fw < 1 || fw > 16384 || fh < 1 || fh > 16384) return AMDAT_SIZE_MISMATCH;
      const amdAprilTagsSize_t& t = D->resize_sizes[RESIZE_SIZE_OF_SLOT(i, nsizes)];   // (tools_hooks.h: i % nsizes)
      fw = t.width; fh = t.height;
    }
    if (!D->per_frame_sizes) {
      if (fw != D->cfg.width || fh != D->cfg.height) return AMDAT_SIZE_MISMATCH;
    } else {   // any size up to the handle's whose working image has a full threshold tile in both directions
      if (fw < 1 || fw > D->cfg.width || fh < 1 || fh > D->cfg.height) return AMDAT_SIZE_MISMATCH;
      const uint32_t w = 1 + (fw - 1) / D->cfg.decimate, h = 1 + (fh - 1) / D->cfg.decimate;
      if (w < D->cfg.tile_size || h < D->cfg.tile_size) return AMDAT_SIZE_MISMATCH;
    }
    if (images[i].pitch < (size_t)images[i].width * enc_channels(fmt)) return AMDAT_INVALID_ARGUMENT;
    if (raw_is_16(fmt) && (((uintptr_t)images[i].dev_ptr | images[i].pitch) & 1u)) return AMDAT_INVALID_ARGUMENT;   // (aligned 16-bit loads)
    if (raw_is_bayer(fmt) && (images[i].width < 2 || images[i].height < 2)) return AMDAT_SIZE_MISMATCH;   // (the reflect rule)
    if ((uint64_t)images[i].pitch * images[i].height > 0x7FFFFFFFull) return AMDAT_INVALID_ARGUMENT;   // 32-bit pixel offsets on the device
    if (images[i].pitch >= (1u << 24)) return AMDAT_INVALID_ARGUMENT;   // (row offsets are formed with 24-bit multiplies: a 16 MB row is no image)
  }
  return AMDAT_SUCCESS;
}

// A colour submission takes the fused loader of the one-pass threshold kernel where that kernel runs undecimated (tile_size 4,
// decimate 1: the reference's cuAprilTags configuration); otherwise one conversion launch ahead of the mono8 pipeline.
static inline bool colour_fused(const amdAprilTagsDetector_st* D, uint32_t fmt) {
  return fmt != AMDAT_ENC_MONO8 && D->P.decimate == 1 && D->P.tile == 4;
}
// The working-size gray plane at decimate 1 (decimated handles have it from creation): allocated on first use by a colour submission
// that takes the fused loader, or by amdAprilTagsSetQuadSigma for the filtered image.
static int ensure_gray_plane(amdAprilTagsDetector_st* D) {
  if (D->d_gray) return AMDAT_SUCCESS;
  const size_t bytes = (size_t)D->cfg.max_batch * D->P.H * D->P.WS;
  if (!dev_alloc(D, D->d_gray, bytes)) return AMDAT_OUT_OF_MEMORY;
  if (hipMemsetAsync(D->d_gray, 0, bytes, D->own_stream) != hipSuccess || hipStreamSynchronize(D->own_stream) != hipSuccess) return AMDAT_HIP_ERROR;
  return AMDAT_SUCCESS;
}
// The gray plane the colour frames of a submission become (allocated on the first colour submission; the pointers travel
// through the descriptor block, so captured launch sequences of earlier mono8 submissions stay valid).
// (filt: the submission runs the quad_sigma filter.  At decimate 1 the filter reads the colour frame itself and writes d_gray, which the
// setter has allocated: no plane here.)
static int ensure_colour_plane(amdAprilTagsDetector_st* D, uint32_t fmt, bool filt = false) {
  if (fmt == AMDAT_ENC_MONO8 || (filt && D->P.decimate == 1)) return AMDAT_SUCCESS;
  return colour_fused(D, fmt) ? ensure_gray_plane(D) : ensure_conv_plane(D);
}

static void fill_frames(amdAprilTagsDetector_st* D, uint32_t n, const amdAprilTagsImageInput_t* images,
                        const amdAprilTagsCameraIntrinsics_t* intr, uint32_t fmt = AMDAT_ENC_MONO8, bool filt = false) {
  for (uint32_t i = 0; i < n; i++) {
    const amdAprilTagsCameraIntrinsics_t& k = intr ? intr[i] : D->cfg.intrinsics;
    if (filt && D->P.decimate == 1) {   // quad_sigma at decimate 1: every stage reads the filtered plane, the filter reads `src`
      D->h_frames[i].img = D->d_gray + (size_t)i * D->P.H * D->P.WS;
      D->h_frames[i].pitch = (uint32_t)D->P.WS;
      D->h_frames[i].src = images[i].dev_ptr;
      D->h_frames[i].src_pitch = (uint32_t)images[i].pitch;
    } else if (fmt == AMDAT_ENC_MONO8) {
      D->h_frames[i].img = images[i].dev_ptr;
      D->h_frames[i].pitch = (uint32_t)images[i].pitch;
      D->h_frames[i].src = nullptr; D->h_frames[i].src_pitch = 0;
    } else {   // every stage behind the threshold pass (or the conversion launch) reads the handle's gray plane
      const bool fused = colour_fused(D, fmt);
      D->h_frames[i].img = fused ? D->d_gray + (size_t)i * D->P.H * D->P.WS : conv_slot(D, i);
      D->h_frames[i].pitch = fused ? (uint32_t)D->P.WS : (uint32_t)D->conv_pitch;
      D->h_frames[i].src = images[i].dev_ptr;
      D->h_frames[i].src_pitch = (uint32_t)images[i].pitch;
    }
    D->h_frames[i].fmt = fmt;
    D->h_frames[i].seq = D->seq;
    {   // the frame's extents and what the algorithm derives from them (check_images: the handle's own size unless per_frame_sizes)
      FrameDesc& fd = D->h_frames[i];
      fd.W0 = (int32_t)images[i].width; fd.H0 = (int32_t)images[i].height;
      fd.W = 1 + (fd.W0 - 1) / D->P.decimate; fd.H = 1 + (fd.H0 - 1) / D->P.decimate;
      fd.wh = (uint32_t)fd.W | ((uint32_t)fd.H << 16);
      fd.tw = fd.W / D->P.tile; fd.th = fd.H / D->P.tile;
      fd.max_cluster_points = 3 * (2 * fd.W + 2 * fd.H);
    }
    D->h_frames[i].fx = (double)k.fx; D->h_frames[i].fy = (double)k.fy;
    D->h_frames[i].cx = (double)k.cx; D->h_frames[i].cy = (double)k.cy;
    D->h_frames[i].skew = (double)(i < D->frame_skew.size() ? D->frame_skew[i] : D->cfg.skew);
  }
}

// A Bayer or 16-bit submission (raw_formats.h): the plane d_raw at the largest source size seen so far -- allocated here by the first
// such submission, regrown here when a larger source arrives (nothing is in flight: begin_batch) -- the descriptors of the conversion
// launch, and the plane's slots as the mono8 images the rest of the submission is filled from.  nullptr: the plane could not be allocated.
static const amdAprilTagsImageInput_t* fill_raw(amdAprilTagsDetector_st* D, uint32_t n, const amdAprilTagsImageInput_t* images, uint32_t fmt) {
  const size_t B = D->cfg.max_batch;
  if (!ensure_dev(D, D->d_rawdesc, B * sizeof(RawDesc)) || !ensure_host(D, D->h_rawdesc, B * sizeof(RawDesc))) return nullptr;
  D->raw_imgs.resize(B);
  uint32_t mw = D->raw_w, mh = D->raw_h;
  for (uint32_t i = 0; i < n; i++) { mw = std::max(mw, images[i].width); mh = std::max(mh, images[i].height); }
  if (!D->d_raw || mw > D->raw_w || mh > D->raw_h) {
    const size_t pitch = ((size_t)mw + 63) & ~(size_t)63;
    if (!dev_regrow(D, D->d_raw, B * pitch * mh)) return nullptr;
    D->raw_pitch = pitch; D->raw_w = mw; D->raw_h = mh;
  }
  for (uint32_t i = 0; i < n; i++) {
    RawDesc& r = D->h_rawdesc[i];
    r.src = images[i].dev_ptr;
    r.dst = D->d_raw + (size_t)i * D->raw_pitch * D->raw_h;
    r.src_pitch = (uint32_t)images[i].pitch; r.dst_pitch = (uint32_t)D->raw_pitch;
    r.enc = fmt; r.shift = D->raw_shift;
    r.w = (int32_t)images[i].width; r.h = (int32_t)images[i].height;
    r.store = RAW_STORE_PLANE; r.pad = 0;
    D->raw_imgs[i] = {images[i].width, images[i].height, r.dst, D->raw_pitch};
  }
  return D->raw_imgs.data();
}

// Rectification or resize on: the descriptors of the front kernel for the caller's frames (encoding fmt) -- each slot's target size,
// which is its own where the resize is off, and its camera where rectification is on -- and the plane's slots at those sizes as the
// mono8 images the rest of the submission is filled from.
static const amdAprilTagsImageInput_t* fill_front(amdAprilTagsDetector_st* D, uint32_t n, const amdAprilTagsImageInput_t* images, uint32_t fmt) {
  const uint32_t nsizes = (uint32_t)D->resize_sizes.size(), ncams = (uint32_t)D->rect_models.size();
  for (uint32_t i = 0; i < n; i++) {
    amdAprilTagsSize_t t = {images[i].width, images[i].height};
    if (nsizes) t = D->resize_sizes[RESIZE_SIZE_OF_SLOT(i, nsizes)];   // (tools_hooks.h: i % nsizes)
    FrontDesc& f = D->h_front[i];
    f.src = images[i].dev_ptr;
    f.src_pitch = (uint32_t)images[i].pitch;
    f.dst = conv_slot(D, i);
    f.dst_pitch = (uint32_t)D->conv_pitch;
    f.fmt = fmt;
    f.SW = (int32_t)images[i].width; f.SH = (int32_t)images[i].height;
    f.DW = (int32_t)t.width; f.DH = (int32_t)t.height;
    f.rectify = ncams ? 1u : 0u;
    if (ncams) camera_model_params(D->rect_models[RECT_MODEL_OF_SLOT(i, ncams)], f.model, f.gen);   // (tools_hooks.h: i % ncams)
    D->front_imgs[i] = {t.width, t.height, f.dst, D->conv_pitch};
  }
  return D->front_imgs.data();
}

// The quad_sigma filter of a submission: each frame's working image (decimate 1: `src`, mono8 or colour; otherwise `img` sampled at the
// decimation) filtered into its slot of d_gray.
static void launch_quad_sigma(amdAprilTagsDetector_st* D, const DetParams& P, uint32_t n, hipStream_t s, uint32_t fmt) {
  QsTaps T = D->qs;
  T.kind = P.decimate == 1 ? (int)fmt : 3 + (P.decimate < 4 ? P.decimate : 4);
  const int gx = (P.W + QS_TW - 1) / QS_TW, gy = (P.H + QS_TH - 1) / QS_TH;
  const unsigned ntiles = (unsigned)gx * gy * n;
  const dim3 grid(8u * ((ntiles + 7u) / 8u));
  switch (D->qs_kh) {   // (the kernel takes every extent from the frame's descriptor; P carries strides)
    case 1: hipLaunchKernelGGL(k_quad_sigma<1>, grid, dim3(256), 0, s, D->d_frames, D->d_gray, gx, gy, (int)n, T, P); break;
    case 2: hipLaunchKernelGGL(k_quad_sigma<2>, grid, dim3(256), 0, s, D->d_frames, D->d_gray, gx, gy, (int)n, T, P); break;
    case 4: hipLaunchKernelGGL(k_quad_sigma<4>, grid, dim3(256), 0, s, D->d_frames, D->d_gray, gx, gy, (int)n, T, P); break;
    default: hipLaunchKernelGGL(k_quad_sigma<8>, grid, dim3(256), 0, s, D->d_frames, D->d_gray, gx, gy, (int)n, T, P); break;
  }
}

// filt: the submission runs the quad_sigma filter (the handle's setting; amdAprilTagsThresholdOnly never does).  The filter goes first,
// and the threshold pass then reads the filtered plane at decimate 1 over W x H (the PLANE instances) and leaves it as it is.
static void launch_threshold(amdAprilTagsDetector_st* D, const DetParams& P, uint32_t n, hipStream_t s, uint32_t fmt = AMDAT_ENC_MONO8,
                             bool filt = false) {
  // conversion launch: src -> the full-size mono8 plane the descriptors name (with the filter at decimate 1 the filter reads the colour
  // frame itself; at decimate > 1 decode reads the conversion plane and the filter samples it)
  if (fmt != AMDAT_ENC_MONO8 && (filt ? P.decimate > 1 : !colour_fused(D, fmt))) {
    const dim3 g((P.W0 + 1023) / 1024, (unsigned)P.H0, n);
    switch (fmt) {
      case AMDAT_ENC_RGB8: hipLaunchKernelGGL((k_to_mono8_frames<3, 0, 2>), g, dim3(256), 0, s, D->d_frames); break;
      case AMDAT_ENC_BGR8: hipLaunchKernelGGL((k_to_mono8_frames<3, 2, 0>), g, dim3(256), 0, s, D->d_frames); break;
      case AMDAT_ENC_RGBA8: hipLaunchKernelGGL((k_to_mono8_frames<4, 0, 2>), g, dim3(256), 0, s, D->d_frames); break;
      default: hipLaunchKernelGGL((k_to_mono8_frames<4, 2, 0>), g, dim3(256), 0, s, D->d_frames); break;
    }
    fmt = AMDAT_ENC_MONO8;
  }
  if (filt) launch_quad_sigma(D, P, n, s, fmt);
  if (P.tile != 4) {   // the two-pass statement (kernels_threshold.h); 4 keeps the one-pass kernel below
    const dim3 g1((unsigned)((P.tw * P.th + 255) / 256), 1, n), g2((unsigned)((P.W + 255) / 256), (unsigned)P.H, n);
#define TH_ANY(DEC, PLANE)                                                                                                       \
    hipLaunchKernelGGL((k_tile_minmax<DEC, PLANE>), g1, dim3(256), 0, s, D->d_frames, D->d_tmin, D->d_tmax, P.tile, P, D->d_gray);  \
    hipLaunchKernelGGL((k_threshold_any_tile<DEC, PLANE>), g2, dim3(256), 0, s, D->d_frames, D->d_gray, D->d_thr, D->d_tmin, D->d_tmax, P.tile, P);
    if (filt) { TH_ANY(1, true) }
    else switch (P.decimate) {
      case 1: TH_ANY(1, false) break;
      case 2: TH_ANY(2, false) break;
      case 3: TH_ANY(3, false) break;
      default: TH_ANY(4, false) break;
    }
#undef TH_ANY
    return;
  }
  const int gx = ((P.W + 3) / 4 + TH_BTX - 1) / TH_BTX, gy = ((P.H + 3) / 4 + TH_BTY - 1) / TH_BTY;
  const unsigned ntiles = (unsigned)gx * gy * n;
  dim3 grid(8u * ((ntiles + 7u) / 8u));
  // the pixels right of / below the last full tile: the handle's own remainder, or -- per-frame sizes -- what any admissible frame
  // can have, up to three columns and three rows (threads beyond a frame's own count return)
  const bool leftover = D->per_frame_sizes || (P.W % 4) || (P.H % 4);
  const int nleft = D->per_frame_sizes ? 3 * (P.W + P.H) : (P.W - P.tw * 4) * (P.th * 4) + (P.H - P.th * 4) * P.W;
  dim3 lgrid((unsigned)((nleft + 255) / 256), 1, n);
#define TH_LAUNCH(DEC, FMT, PLANE)                                                                                                  \
  hipLaunchKernelGGL((k_threshold<DEC, FMT, PLANE>), grid, dim3(256), 0, s, D->d_frames, D->d_gray, D->d_thr, gx, gy, (int)n, P);    \
  if (leftover) hipLaunchKernelGGL((k_threshold_leftover<DEC, FMT, PLANE>), lgrid, dim3(256), 0, s, D->d_frames, D->d_gray, D->d_thr, P);
  if (filt) {
    TH_LAUNCH(1, 0, true)
    return;
  }
  if (fmt != AMDAT_ENC_MONO8) {   // (decimate 1: colour_fused)
    switch (fmt) {
      case AMDAT_ENC_RGB8: TH_LAUNCH(1, 1, false) break;
      case AMDAT_ENC_BGR8: TH_LAUNCH(1, 2, false) break;
      case AMDAT_ENC_RGBA8: TH_LAUNCH(1, 3, false) break;
      default: TH_LAUNCH(1, 4, false) break;
    }
    return;
  }
  switch (P.decimate) {
    case 1: TH_LAUNCH(1, 0, false) break;
    case 2: TH_LAUNCH(2, 0, false) break;
    case 3: TH_LAUNCH(3, 0, false) break;
    default: TH_LAUNCH(4, 0, false) break;
  }
#undef TH_LAUNCH
}

// first launch of a submission: frame descriptors from the pinned host block to device memory, work-list control words
// and frame counters to zero (one block per frame)
__global__ __launch_bounds__(64) void k_prologue(const uint32_t* __restrict__ host_frames, uint32_t* __restrict__ frames,
                                                 uint32_t* __restrict__ workctl, uint32_t* __restrict__ counters, int fd_words, int fc_words,
                                                 const uint32_t* __restrict__ host_front, uint32_t* __restrict__ front, int front_words,
                                                 const uint32_t* __restrict__ host_ucams, uint32_t* __restrict__ ucams, int ucam_words,
                                                 const uint32_t* __restrict__ host_rig, uint32_t* __restrict__ rig, int rig_words,
                                                 const uint32_t* __restrict__ host_raw, uint32_t* __restrict__ raw, int raw_words) {
  const int frame = (int)blockIdx.x, t = (int)threadIdx.x;
  for (int i = t; i < fd_words; i += 64) frames[frame * fd_words + i] = host_frames[frame * fd_words + i];
  for (int i = t; i < front_words; i += 64) front[frame * front_words + i] = host_front[frame * front_words + i];   // (no front stage: no words)
  for (int i = t; i < ucam_words; i += 64) ucams[frame * ucam_words + i] = host_ucams[frame * ucam_words + i];   // (no corner undistortion: no words)
  for (int i = t; i < rig_words; i += 64) rig[frame * rig_words + i] = host_rig[frame * rig_words + i];   // (no camera rig: no words)
  for (int i = t; i < raw_words; i += 64) raw[frame * raw_words + i] = host_raw[frame * raw_words + i];   // (no raw conversion: no words)
  for (int i = t; i < fc_words; i += 64) counters[frame * fc_words + i] = 0u;
  if (frame == 0 && t < 32) workctl[t] = 0u;
}

// k_reconcile writes every frame's records and counters straight into the pinned host buffers the API call reads: no copy commands
// after the last kernel (about 10 us of a one-frame call; at 256 frames the strided 3.8 MB copy of mostly empty record slots cost
// 0.08 ms per step against the ~0.6 MB of real records the kernel writes: 17.85 -> 17.77 ms).

// Enqueues the stage sequence of plan_launch (launch_plan.h) for batch slots [0, n) on stream s.  mark() is called between stages
// (event timing when profiling).
static int issue_pipeline(amdAprilTagsDetector_st* D, uint32_t n, uint32_t ostride, hipStream_t s, uint32_t fmt, const std::function<void()>& mark) {
  DetParams P = D->P;
  P.frame0 = 0;
  const LaunchPlan plan = plan_launch(D->fq, n, P.W, P.H, P.hcap, D->path_mode, (unsigned)D->num_cus, FQ_SOUND_EXIT_PREFILTER);
  launch_threshold(D, P, n, s, fmt, D->qs_ksz > 1);
  mark();
  {
    const dim3 grid((P.W + CC_T - 1) / CC_T, (P.H + CC_T - 1) / CC_T, n);
    if (plan.cc_waves == 16)
      hipLaunchKernelGGL((k_cc_local<16>), grid, dim3(1024), 0, s, D->d_thr, D->d_label, D->d_csize, D->d_roots, D->d_perim, D->d_counters, D->d_frames, P);
    else
      hipLaunchKernelGGL((k_cc_local<4>), grid, dim3(256), 0, s, D->d_thr, D->d_label, D->d_csize, D->d_roots, D->d_perim, D->d_counters, D->d_frames, P);
  }
  mark();
  {
    const int nrows = (P.H - 1) / CC_T, ncols = (P.W - 1) / CC_T;
    const long total = (long)nrows * P.W + (long)ncols * P.H;
    if (total > 0) {
#define BORDER_ARGS dim3((unsigned)((total + 255) / 256) * n), dim3(256), 0, s, D->d_perim, D->d_label, D->d_roots, D->d_counters,   \
                    (uint32_t)((total + 255) / 256), n, D->d_frames, P
      if (plan.border_per_wave) hipLaunchKernelGGL((k_cc_border<true>), BORDER_ARGS);
      else hipLaunchKernelGGL((k_cc_border<false>), BORDER_ARGS);
#undef BORDER_ARGS
    }
  }
  mark();
  hipLaunchKernelGGL(k_cc_sizes, dim3(plan.cc_root_grid, 1, n), dim3(256), 0, s, D->d_label, D->d_csize, D->d_roots, D->d_counters, P);
  hipLaunchKernelGGL(k_cc_resolve, dim3(plan.cc_root_grid, 1, n), dim3(256), 0, s, D->d_label, D->d_csize, D->d_roots, D->d_counters, P);
  mark();
  const uint32_t gxt = (uint32_t)((P.W + PT_TW - 1) / PT_TW), gyt = (uint32_t)((P.H + PT_TH - 1) / PT_TH);
  hipLaunchKernelGGL(k_points, dim3(gxt * gyt * n), dim3(256), 0, s, D->d_thr, D->d_label, D->d_hkeys, D->d_hcnt,
                     D->d_stage, D->d_bhdr, D->d_btab, D->d_long, D->d_counters, (D->fq_counters ? D->d_ptprof : nullptr), gxt, gyt, n, D->d_frames, P);
  mark();
  const FqWorkLayout& L = D->work_layout.all;
  hipLaunchKernelGGL(k_cluster_select, dim3(plan.select_grid, 1, n), dim3(256), 0, s, D->d_hkeys, D->d_hcnt, D->d_hoff, D->d_clusters,
                     D->d_counters, D->d_work, D->d_workctl, plan.latency ? D->work_layout.latency : L, plan.select_chunks, D->d_frames, P);
  mark();
  hipLaunchKernelGGL(k_scatter, dim3((gxt * gyt + 3) / 4, 1, n), dim3(256), 0, s, D->d_stage, D->d_bhdr, D->d_btab, D->d_long, D->d_hoff, D->d_pts,
                     D->d_counters, gxt, gyt, P);
  mark();
  {
    // the prefilter's compact lists (d_work2, counts at d_workctl + 16), indexed with the common layout
    uint32_t* const work2 = D->d_work2 - L.off[D->fq.prefilter_class];
    const hipStream_t* aux = D->aux_stream;
    for (int i = 0; i < plan.nsteps; i++) {
      const FitStep& st = plan.steps[i];
      const hipStream_t sc = st.stream == FIT_MAIN ? s : aux[st.stream];
      const dim3 grid(st.grid);
      if (st.kind == FIT_FORK) {
        HIP_TRY(hipEventRecord(D->ev_fork, s));
        for (int a = 0; a < FQ_NAUX; a++) HIP_TRY(hipStreamWaitEvent(aux[a], D->ev_fork, 0));
      } else if (st.kind == FIT_PREFILTER) {
        if (FQ_SKIP_PREFILTER()) continue;   // (tools_hooks.h: always 0 in the product build)
#define PF_ARGS D->d_frames, D->d_gray, D->d_pts, D->d_clusters, D->d_work, D->d_workctl, work2, D->d_workctl + 16, D->d_workctl + 24,   \
                L, plan.prefilter_first, (D->fq_counters ? D->d_fqprof : nullptr), P
        if (plan.prefilter_nt == 1024) hipLaunchKernelGGL(k_fit_prefilter<1024>, grid, dim3(1024), 0, sc, PF_ARGS);
        else hipLaunchKernelGGL(k_fit_prefilter<64>, grid, dim3(64), 0, sc, PF_ARGS);
#undef PF_ARGS
      } else {
        const int c = st.cls;
        if (FQ_SKIP_CLASS(c)) continue;   // (tools_hooks.h: always 0 in the product build)
        const FqClassSpec& cl = D->fq.cls[c];
        const FqScratch& scr = D->fq_scratch[c];
        if (cl.kernel == FQ_SMALL) {
          hipLaunchKernelGGL(k_fit_small<2>, grid, dim3(64), FS_LDS_BYTES(2), sc, D->d_frames, D->d_gray, D->d_pts, D->d_clusters,
                             D->d_work + L.off[c], D->d_workctl + c, L.cap[c], D->d_workctl + 8 + c, D->d_cands, D->d_counters, st.pop, P);
          continue;
        }
        const size_t lds = FQ_LDS_BYTES(cl.nt, cl.sort_cap);   // (kernels_quad.h: the kernel's dynamic-LDS layout)
#define FQ_ARGS D->d_frames, D->d_gray, D->d_pts, D->d_clusters, (st.compact ? work2 : D->d_work) + L.off[c],                       \
                D->d_workctl + (st.compact ? 16 : 0) + c, L.cap[c], D->d_workctl + 8 + c, scr.d_lf,                                \
                (c == FQ_NCLS - 1 ? D->d_keys_scr : nullptr), scr.d_errs, D->d_cands, D->d_counters,                               \
                (D->fq_counters ? D->d_fqprof + 8 * (c - FQ_C0) : nullptr), cl.sort_cap, cl.slot_cap, st.pop, P
#define FQ_LAUNCH(NTV)                                                                                          \
  if (P.split_moments) hipLaunchKernelGGL((k_fit_quads<NTV, true>), grid, dim3(NTV), lds, sc, FQ_ARGS);          \
  else hipLaunchKernelGGL((k_fit_quads<NTV, false>), grid, dim3(NTV), lds, sc, FQ_ARGS);
        if (cl.nt == 64) { FQ_LAUNCH(64) }
        else if (cl.nt == 128) { FQ_LAUNCH(128) }
        else if (cl.nt == 256) { FQ_LAUNCH(256) }
        else if (cl.nt == 512) { FQ_LAUNCH(512) }
        else { FQ_LAUNCH(FQ_NT_BIG) }
#undef FQ_LAUNCH
#undef FQ_ARGS
      }
    }
    for (int a = 0; a < FQ_NAUX; a++) {
      HIP_TRY(hipEventRecord(D->ev_join[a], aux[a]));
      HIP_TRY(hipStreamWaitEvent(s, D->ev_join[a], 0));
    }
    // corners + area / angle checks of the candidates, one thread each
    hipLaunchKernelGGL(k_quad_finish, dim3(16, n), dim3(256), 0, s, D->d_cands, D->d_quads, D->d_counters, P);
  }
  mark();
  hipLaunchKernelGGL(k_decode_wave, dim3(plan.decode_grid, n), dim3(64), 0, s, D->d_frames, D->d_quads, D->d_dets, D->d_counters,
                     DECODE_PARAMS(P, D->qs_ksz > 1));   // (tools_hooks.h: P in the product build)
  mark();
  hipLaunchKernelGGL(k_reconcile, dim3(n), dim3(64), 0, s, D->d_frames, D->d_dets, D->d_counters, D->d_order, D->h_out, ostride,
                     D->h_counters, P, (const void*)D->d_tag_table.p);
  // The stages behind k_reconcile, as plan_post lists them (post_plan.h), one wave per block except the rigid kind's two
  const PostPlan post = plan_post(D->last.post, n, ostride);
  for (int i = 0; i < post.nsteps; i++) {
    const PostStep& st = post.steps[i];
    const dim3 grid(st.gx, st.gy);
    // raw-frame mode: the pose launches read the twins, which order and count as the raw records do (tools_hooks.h: d_dets_u in the product build)
    const DetRec* const pose_dets = st.twins ? UD_POSE_RECORDS(D->d_dets, D->d_dets_u) : D->d_dets;
#define RIGID_LAUNCH(COV)                                                                                                          \
  hipLaunchKernelGGL(k_bundle_rigid<COV>, grid, dim3(128), 0, s, D->d_frames, pose_dets, D->d_counters, D->d_order, D->d_rigid_head, \
                     D->d_rigid_members, D->d_rigid_table, D->h_xposes, P, (const double*)D->d_cov_cfg, (PoseCovRec*)D->h_xcovs)
#define POSE_LAUNCH(COV)                                                                                                           \
  hipLaunchKernelGGL(k_pose_refine<COV>, grid, dim3(64), 0, s, D->d_frames, pose_dets, D->d_counters, D->d_order, D->d_pose_cfg,    \
                     D->h_rposes, ostride, P, (const double*)D->d_cov_cfg, (PoseCovRec*)D->h_rcovs, (const void*)D->d_tag_table.p)
    switch (st.kernel) {
      case POST_K_UNDISTORT:   // S9b: the undistorted twin of every kept record (kernels_undistort.h)
        hipLaunchKernelGGL(k_undistort_records, grid, dim3(64), 0, s, D->d_frames, D->d_dets, D->d_counters, D->d_order, D->d_ucams,
                           D->d_dets_u, D->h_udets, ostride, P, (const void*)D->d_tag_table.p);
        break;
      case POST_K_PLANAR:      // S10: one wave per (frame, bundle) on the kept records (kernels_bundle.h)
        hipLaunchKernelGGL(k_bundle_pose, grid, dim3(64), 0, s, D->d_frames, pose_dets, D->d_counters, D->d_order, D->d_bundle_head,
                           D->d_bundle_members, D->d_bundle_table, D->h_bposes, P);
        break;
      case POST_K_RIGID:       // S12: two waves per (frame, bundle), one chain each, in the planar kind's place (kernels_rigid.h)
        if (st.cov) RIGID_LAUNCH(true); else RIGID_LAUNCH(false);
        break;
      case POST_K_REFINE:      // S11: both minima of the records handed out, eight lanes per record (kernels_pose.h)
        if (st.cov) POSE_LAUNCH(true); else POSE_LAUNCH(false);
        break;
      case POST_K_RIG:         // S13: two waves per (group, bundle) over the records of all the group's frames (kernels_rig.h)
        hipLaunchKernelGGL(k_bundle_rig, grid, dim3(128), 0, s, D->d_frames, pose_dets, D->d_counters, D->d_order, D->d_rigid_head,
                           D->d_rigid_members, D->d_rigid_table, D->d_rig, D->h_gposes, P);
        break;
    }
#undef RIGID_LAUNCH
#undef POSE_LAUNCH
  }
  mark();
  return AMDAT_SUCCESS;
}

// Everything one submission enqueues on stream s (and the auxiliary streams forked from it): descriptor upload, clears,
// the stage sequence, result download.  No host synchronisation inside, so the sequence can be stream-captured.
static int enqueue_submission(amdAprilTagsDetector_st* D, uint32_t n, uint32_t ostride, hipStream_t s, uint32_t fmt, const std::function<void()>& mark) {
  // (the snapshot begin_batch took: a regrowth relaunch resizes and rectifies again)
  const bool resize = D->last.resized, rect = D->last.rectified;
  mark();
  // descriptor upload + clears in one small kernel (it reads the pinned descriptor block over the bus itself): a copy
  // command and a fill command ahead of the first kernel cost a one-frame call about 15 us, this launch 4
  static_assert(sizeof(FrameDesc) % 4 == 0 && sizeof(FrameDesc) <= 256 && sizeof(FrameCounters) % 4 == 0 && sizeof(FrameCounters) <= 256, "k_prologue: one word per thread");
  hipLaunchKernelGGL(k_prologue, dim3(n), dim3(64), 0, s, static_cast<const uint32_t*>(D->h_frames.p),
                     static_cast<uint32_t*>(D->d_frames.p), D->d_workctl, reinterpret_cast<uint32_t*>(D->d_counters),
                     (int)(sizeof(FrameDesc) / 4), (int)(sizeof(FrameCounters) / 4),
                     static_cast<const uint32_t*>(D->h_front.p), static_cast<uint32_t*>(D->d_front.p),
                     resize || rect ? (int)(sizeof(FrontDesc) / 4) : 0,
                     static_cast<const uint32_t*>(D->h_ucams.p), static_cast<uint32_t*>(D->d_ucams.p),
                     D->last.post.nundist ? (int)(sizeof(UndistortCam) / 4) : 0,
                     reinterpret_cast<const uint32_t*>(D->h_rig.p), reinterpret_cast<uint32_t*>(D->d_rig.p),
                     D->last.post.nrig ? (int)(sizeof(RigSlotDev) / 4) : 0,
                     reinterpret_cast<const uint32_t*>(D->h_rawdesc.p), reinterpret_cast<uint32_t*>(D->d_rawdesc.p),
                     D->last.raw ? (int)(sizeof(RawDesc) / 4) : 0);
  // raw formats: the first launch behind the descriptors turns the caller's Bayer or 16-bit frames into the mono8 slots of d_raw that the
  // descriptors name (a regrowth relaunch converts again).  The grid is the handle's size: its blocks stride over a larger source.
  if (D->last.raw) {
    const dim3 g((D->cfg.width + RAW_BW - 1) / RAW_BW, (D->cfg.height + RAW_BH - 1) / RAW_BH, n);
    switch (D->last.raw) {
      case RAW_KIND_BAYER8: hipLaunchKernelGGL(k_raw_to_mono8_frames<RAW_KIND_BAYER8>, g, dim3(256), 0, s, D->d_rawdesc); break;
      case RAW_KIND_MONO16: hipLaunchKernelGGL(k_raw_to_mono8_frames<RAW_KIND_MONO16>, g, dim3(256), 0, s, D->d_rawdesc); break;
      default: hipLaunchKernelGGL(k_raw_to_mono8_frames<RAW_KIND_BAYER16>, g, dim3(256), 0, s, D->d_rawdesc); break;
    }
  }
  if (D->fq_counters) HIP_TRY(hipMemsetAsync(D->d_fqprof, 0, (64 + 8) * 8, s));
  // rectification: the caller's frames, whatever their encoding, become the mono8 slots of the rectified plane the descriptors name
  // (the grid is the handle's size; blocks beyond a frame's own extent return)
  // resize: the same, at each slot's target size, through the rectification where that is on (in place of k_rectify_frames)
  // Either way ONE front launch: where some camera of the handle is not plumb_bob with R = I, the kernel that also holds the general
  // projection (it switches per slot, as on the encoding); otherwise today's, whose registers and occupancy stay what they were.
  // (Which of the two is part of a captured graph's key: a change of models retires nothing.)
  const bool general = D->rect_general && !D->rect_models.empty();
  if (resize)
    hipLaunchKernelGGL(general ? k_resize_frames_general : k_resize_frames, dim3((D->cfg.width + RF_BW - 1) / RF_BW, (D->cfg.height + RF_BH - 1) / RF_BH, n), dim3(256), 0, s,
                       D->d_front);
  else if (rect)
    hipLaunchKernelGGL(general ? k_rectify_frames_general : k_rectify_frames, dim3((D->cfg.width + RF_BW - 1) / RF_BW, (D->cfg.height + RF_BH - 1) / RF_BH, n), dim3(256), 0, s,
                       D->d_front);
  mark();
  {
    const int rc = issue_pipeline(D, n, ostride, s, fmt, mark);
    if (rc) return rc;
  }
  mark();
  return AMDAT_SUCCESS;
}

// An instantiated graph that is no longer wanted -- a capacity grew (its launches carry the old pointers), the cache evicted it,
// the submission path was pinned -- is RETIRED, not destroyed.  Root cause (round 6): hipGraphExecDestroy
// followed, with no device-wide wait in between, by the capture, instantiation and launch of the next graph crashes inside
// hipGraphLaunch -- a null node pointer in the runtime's walk over the new graph's nodes -- on the HIP runtime 7.0.51831 that
// PyTorch 2.10.0+rocm7.0 bundles (torch/lib/libamdhip64.so: the runtime every Python process of this repository binds, tests and
// bench included), and NOT on the system's ROCm 7.2.0 runtime the C and C++ hosts link.  tools/repro_graph_regrow.hip is the
// reproducer without library code: `repro_graph_regrow 400 destroy_nosync 3 16` dies with the same runtime frames on PyTorch's
// runtime and completes on ROCm 7.2's.  With the destroy taken out of the way -- retired graphs die with the handle, after its
// device-wide wait and with no capture behind them -- re-capturing on regrown buffers is clean (tools/stress_regrow.py with
// replay kept: 15 of 15 runs of 150 handles; with hipGraphExecDestroy at the regrowth: 11 of 12 runs die), so a regrown handle
// keeps graph replay: the next submission of each shape is captured again on the new buffers.  The list is bounded: beyond
// kMaxRetiredGraphs the handle stops capturing new graphs (plain enqueues for the submission shapes it has no graph for;
// it says so once on stderr and through amdAprilTagsDebugGraphReplay).
constexpr size_t kMaxRetiredGraphs = 24;
static void retire_graph(amdAprilTagsDetector_st* D, amdAprilTagsDetector_st::GraphEntry& g) {
  if (!g.exec) return;
  D->retired_graphs.push_back(g.exec);
  if (D->retired_graphs.size() > kMaxRetiredGraphs && D->graph_max_frames) {
    D->graph_max_frames = 0;   // (the live cache entries keep replaying; nothing new is captured)
    fprintf(stderr, "[apriltag_amd] handle %p: %zu retired launch graphs -- no new graphs are captured from here on (plain enqueues "
                    "for submission shapes without one)\n", (void*)D, D->retired_graphs.size());
  }
  g.exec = nullptr;
}
static void drop_graphs(amdAprilTagsDetector_st* D) {
  for (auto& g : D->graphs) retire_graph(D, g);
}

// After a capture that did not end in a graph: clear the error state and make sure no stream of the handle is left inside the
// dead capture (a side stream that joined it through the fork event and was never joined back stays "capturing": every later
// launch on it would fail with "operation failed due to a previous error during capture") -- such a stream is replaced.
static int recover_from_failed_capture(amdAprilTagsDetector_st* D, hipStream_t s) {
  for (int i = 0; i < 4 && hipGetLastError() != hipSuccess; i++) {}
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone) {
    hipGraph_t g = nullptr;
    (void)hipStreamEndCapture(s, &g);
    if (g) hipGraphDestroy(g);
  }
  for (auto& a : D->aux_stream) {
    st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(a, &st) != hipSuccess || st != hipStreamCaptureStatusNone) {
      (void)hipGetLastError();
      (void)hipStreamDestroy(a);
      a = nullptr;
      if (hipStreamCreateWithFlags(&a, hipStreamNonBlocking) != hipSuccess) return AMDAT_HIP_ERROR;
      // (graphs captured on the old stream object are still valid: a graph holds nodes and edges, not the capture's streams)
    }
  }
  for (int i = 0; i < 4 && hipGetLastError() != hipSuccess; i++) {}
  return AMDAT_SUCCESS;
}

// One pass of a submission over the device: captured-graph replay for small submissions, plain enqueues otherwise.
// launch_once enqueues it and returns; finish_once waits for it (and reads the stage events when profiling is on).
static int launch_once(amdAprilTagsDetector_st* D, uint32_t n, uint32_t ostride, hipStream_t s, uint32_t fmt) {
  D->launched_fmt = fmt;
  D->seq++;
  for (uint32_t i = 0; i < n; i++) D->h_frames[i].seq = D->seq;   // (k_prologue reads the pinned block when the launch executes)
  D->launched_n = n;
  const bool prof = D->profiling;
  D->events_recorded = false;
  D->last_graph_nodes = 0;
  int evi = 0;
  // profiling: one HIP event per stage boundary, and a roctx range per stage (it spans the stage's enqueues; rocprofv3
  // --marker-trace shows them beside the kernels they launched)
  const std::function<void()> mark = [&]() {
    if (!prof) return;
    if (roctx().push) {
      if (evi > 0) roctx().pop();
      if (evi < AMDAT_NUM_STAGES) roctx().push(kStageNames[evi]);
    }
    hipEventRecord(D->ev[evi++], s);
  };
  const std::function<void()> nomark = []() {};

  // Small submissions (the node's one-frame calls) are launch-bound: ~20 enqueues for well under a millisecond of
  // device work.  Their enqueue sequence is captured once per (frames, output stride, stream) into a hipGraph and
  // replayed; everything that changes between calls lives in the descriptor block the graph's first node uploads.  A
  // handful of instantiated graphs is kept (a host that alternates batch sizes or streams would otherwise re-capture on
  // every call, far slower than the plain enqueues the graph replaces); after a few consecutive misses with the cache
  // full, or one failed capture, the handle falls back to plain enqueues for good.
  if (n <= 8 && !prof && D->path_mode != AMDAT_PATH_THROUGHPUT) {
    amdAprilTagsDetector_st::GraphEntry* hit = nullptr;
    for (auto& g : D->graphs)
      if (g.exec && g.n == n && g.ostride == ostride && g.stream == s && g.fmt == fmt && g.general == D->rect_general && g.raw == D->last.raw) hit = &g;
    if (hit) {
      D->graph_misses = 0;
      hit->last_use = ++D->graph_clock;
    } else if (D->graph_max_frames && n <= D->graph_max_frames && D->graph_misses < 8) {
      amdAprilTagsDetector_st::GraphEntry* slot = nullptr;
      for (auto& g : D->graphs) if (!g.exec) { slot = &g; break; }
      if (!slot) {   // evict the least recently used entry
        D->graph_misses++;
        slot = &D->graphs[0];
        for (auto& g : D->graphs) if (g.last_use < slot->last_use) slot = &g;
        retire_graph(D, *slot);   // (not destroyed here: see drop_graphs)
      }
      hipGraph_t graph = nullptr;
      bool ok = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess;
      if (ok) {
        const int rc = enqueue_submission(D, n, ostride, s, fmt, nomark);
        const hipError_t e = hipStreamEndCapture(s, &graph);
        ok = rc == AMDAT_SUCCESS && e == hipSuccess && graph != nullptr;
      }
      size_t nodes = 0;
      if (ok && hipGraphGetNodes(graph, nullptr, &nodes) != hipSuccess) { nodes = 0; (void)hipGetLastError(); }
      if (ok) ok = hipGraphInstantiate(&slot->exec, graph, nullptr, nullptr, 0) == hipSuccess;
      if (graph) hipGraphDestroy(graph);
      if (ok) { slot->n = n; slot->ostride = ostride; slot->fmt = fmt; slot->stream = s; slot->general = D->rect_general; slot->raw = D->last.raw; slot->nodes = (uint32_t)nodes; slot->last_use = ++D->graph_clock; hit = slot; }
      else {
        // A capture can be invalidated from OUTSIDE the library: on this runtime a legacy-stream call of any other host thread on
        // the same device (a plain hipMemcpy) while this thread captures fails that call and poisons the capture, in every capture
        // mode (examples/multi_stream_host --shared-gpu met it with eight threads on one device).  The submission
        // then goes out as plain enqueues -- after the side streams have been taken out of the dead capture -- and the handle
        // tries a capture again on later submissions; three failures end graph replay for the handle.
        slot->exec = nullptr;
        const int crc = recover_from_failed_capture(D, s);
        if (crc) return crc;
        if (++D->capture_failures >= 3) D->graph_max_frames = 0;
      }
    }
    if (hit) {
      D->last_graph_nodes = hit->nodes;
      HIP_TRY(hipGraphLaunch(hit->exec, s));
      return AMDAT_SUCCESS;
    }
  }
  {
    const int rc = enqueue_submission(D, n, ostride, s, fmt, mark);
    if (rc) return rc;
  }
  D->events_recorded = prof;
  HIP_TRY(hipGetLastError());
  return AMDAT_SUCCESS;
}

static int finish_once(amdAprilTagsDetector_st* D, hipStream_t s) {
  HIP_TRY(hipStreamSynchronize(s));
  // The counters the host is about to act on must be THIS launch's: k_reconcile stamps them with the descriptor's sequence number
  // as its last store.  (The regrowth stress loop once ended with a handle that had not grown -- counters read before they were
  // final, under graph replay on ROCm 7.2.)  A mismatch waits for the whole device and looks again; if the results still are not
  // there the call fails instead of handing out an earlier launch's records.
  auto stamped = [&]() {
    for (uint32_t f = 0; f < D->launched_n; f++)
      if (static_cast<volatile FrameCounters*>(D->h_counters)[f].seq != D->seq) return false;
    // The stages behind k_reconcile stamp every record they hand out the same way: the blocks the submission's plan lists (the
    // records' counts are final: the frames' stamps were seen above).  Per PostBlock: where it lies, its record size, the stamp's offset.
    const struct { const void* p; size_t size, seq; } blocks[] = {
        {D->h_udets.p, sizeof(UndistortRec), offsetof(UndistortRec, seq)}, {D->h_bposes.p, sizeof(BundlePoseRec), offsetof(BundlePoseRec, seq)},
        {D->h_xposes.p, sizeof(RigidPoseRec), offsetof(RigidPoseRec, seq)}, {D->h_xcovs.p, sizeof(PoseCovRec), offsetof(PoseCovRec, seq)},
        {D->h_rposes.p, sizeof(PoseRefineRec), offsetof(PoseRefineRec, seq)}, {D->h_rcovs.p, sizeof(PoseCovRec), offsetof(PoseCovRec, seq)},
        {D->h_gposes.p, sizeof(RigPoseRec), offsetof(RigPoseRec, seq)}};
    static_assert(POST_B_UDETS == 0 && POST_B_BPOSES == 1 && POST_B_XPOSES == 2 && POST_B_XCOVS == 3 && POST_B_RPOSES == 4 && POST_B_RCOVS == 5 && POST_B_GPOSES == 6, "blocks[]");
    const PostPlan post = plan_post(D->last.post, D->launched_n, D->last.ostride);
    for (int i = 0; i < post.nsteps; i++)
      for (int j = 0; j < post.steps[i].nwrites; j++) {
        const PostWrite& w = post.steps[i].writes[j];
        const char* const recs = static_cast<const char*>(blocks[w.block].p) + blocks[w.block].seq;
        for (uint32_t f = 0; f < D->launched_n; f++) {
          uint32_t k = w.per_frame;   // POST_BY_BUNDLE: every entry of the frame
          if (w.index == POST_BY_RECORD && D->h_counters[f].nout < k) k = D->h_counters[f].nout;
          for (uint32_t r = 0; r < k; r++)
            if (*reinterpret_cast<const volatile uint32_t*>(recs + ((size_t)f * w.per_frame + r) * blocks[w.block].size) != D->seq) return false;
        }
      }
    return true;
  };
  if (!stamped()) {
    D->late_waits++;
    HIP_TRY(hipDeviceSynchronize());
    if (!stamped()) {
      fprintf(stderr, "[apriltag_amd] launch %u: results missing after a device-wide wait\n", D->seq);
      return AMDAT_HIP_ERROR;
    }
  }
  if (D->events_recorded) {
    for (int i = 0; i < AMDAT_NUM_STAGES; i++) {
      float ms = 0;
      hipEventElapsedTime(&ms, D->ev[i], D->ev[i + 1]);
      D->stage_ms[i] = ms;
    }
  }
  return AMDAT_SUCCESS;
}


// The capacities the growth policy sees (growth.h) and takes back.  P.lcap follows from pcap and lcap_div (alloc_point_buffers).
static GrowCaps caps_of(const amdAprilTagsDetector_st* D) {
  return {D->P.pcap, D->P.lcap, D->P.hcap, D->P.ccap, D->P.qcap, D->P.cand_cap, D->lcap_div};
}
static void set_caps(amdAprilTagsDetector_st* D, const GrowCaps& c) {
  DetParams& P = D->P;
  P.pcap = c.pcap; P.lcap = c.lcap; P.hcap = c.hcap; P.ccap = c.ccap; P.qcap = c.qcap; P.cand_cap = c.cand_cap; D->lcap_div = c.lcap_div;
}

// Reallocates what a growth plan names and takes its capacities; false if an allocation failed.  The cluster, quad and candidate
// lists get their new buffer before the old one goes; the point buffers and the pair table are freed first (alloc_*_buffers), so a
// failure there reallocates them at the old capacities -- and if even that fails the handle is unusable.  Graphs are retired only
// when a buffer changed: their launches carry the old pointers and capacities.
static bool regrow(amdAprilTagsDetector_st* D, const GrowPlan& g) {
  const size_t B = D->cfg.max_batch;
  const GrowCaps before = caps_of(D);
  bool ok = true;
  switch (g.family) {
    case GROW_QUADS: ok = dev_regrow(D, D->d_quads, B * g.caps.qcap * sizeof(QuadRec)); break;
    case GROW_CANDS: ok = dev_regrow(D, D->d_cands, B * g.caps.cand_cap * sizeof(FitCand)); break;
    case GROW_CLUSTERS: {   // the quad fit's work lists are sized from ccap: the point buffers follow
      DevBuf<ClusterRec> old = D->d_clusters;
      D->d_clusters = {};
      if (!dev_alloc(D, D->d_clusters, B * g.caps.ccap * sizeof(ClusterRec))) { D->d_clusters = old; ok = false; break; }
      drop_graphs(D);
      set_caps(D, g.caps);
      ok = alloc_point_buffers(D) == AMDAT_SUCCESS;
      if (ok) { dev_free(D, old); break; }
      dev_free(D, D->d_clusters);   // (the grown list goes before the point buffers are reallocated at the old capacity)
      D->d_clusters = old;
      set_caps(D, before);
      if (alloc_point_buffers(D) != AMDAT_SUCCESS) D->unusable = true;
      break;
    }
    default:   // GROW_POINTS, GROW_HASH (the point buffers also when only the staging format changes)
      drop_graphs(D);
      set_caps(D, g.caps);
      ok = alloc_hash_buffers(D) == AMDAT_SUCCESS && alloc_point_buffers(D) == AMDAT_SUCCESS;
      if (!ok) {
        set_caps(D, before);
        if (alloc_hash_buffers(D) != AMDAT_SUCCESS || alloc_point_buffers(D) != AMDAT_SUCCESS) D->unusable = true;
      }
  }
  if (!ok) return false;
  drop_graphs(D);   // (a no-op where the case above dropped them)
  set_caps(D, g.caps);
  return true;
}

// One batched submission; results land in h_out / h_counters with `ostride` records per frame.
// begin_batch fills the descriptor block and enqueues the submission; end_batch waits for it, and where a frame overflowed a
// capacity the handle may grow, grows it and runs the submission again (the descriptors are still in the pinned block).
static int begin_batch(amdAprilTagsDetector_st* D, uint32_t n, const amdAprilTagsImageInput_t* images,
                       const amdAprilTagsCameraIntrinsics_t* intr, uint32_t ostride, hipStream_t s, uint32_t fmt = AMDAT_ENC_MONO8) {
  if (D->inflight.active) return AMDAT_INVALID_ARGUMENT;   // one submission per handle at a time (amdAprilTagsWaitBatch first)
  DeviceGuard guard(D->device);
  if (!guard.ok) return AMDAT_HIP_ERROR;
  if (D->unusable) return AMDAT_OUT_OF_MEMORY;   // (never launch on the half-allocated buffers of a failed regrowth)
  if (D->post.nrig) { const int rrc = fill_rig(D, n); if (rrc) return rrc; }   // (refused before anything of the submission is written)
  const bool filt = D->qs_ksz > 1;   // (the setter refuses while a submission is in flight: a regrowth relaunch filters the same way)
  const bool resized = !D->resize_sizes.empty(), rectified = !resized && !D->rect_models.empty();   // (resized: the rectified plane is never formed)
  const uint32_t raw = (uint32_t)raw_kind(fmt);
  if (raw) {   // from here on a mono8 submission of the raw plane's slots (the front stage reads them as its mono8 source)
    images = fill_raw(D, n, images, fmt);
    if (!images) return AMDAT_OUT_OF_MEMORY;
    fmt = AMDAT_ENC_MONO8;
  }
  if (resized || rectified) {   // from here on a mono8 submission of the front plane's slots at their target sizes
    images = fill_front(D, n, images, fmt);
    fmt = AMDAT_ENC_MONO8;
  }
  { const int crc = ensure_colour_plane(D, fmt, filt); if (crc) return crc; }
  fill_frames(D, n, images, intr, fmt, filt);   // image pointers, pitches and intrinsics travel through the pinned descriptor block
  D->last_path = latency_set(n, D->P.W, D->P.H, D->path_mode) ? AMDAT_PATH_LATENCY : AMDAT_PATH_THROUGHPUT;
  if (ostride > D->P.dcap) ostride = D->P.dcap;
  D->last = {n, ostride, D->post, rectified, resized, raw};
  for (uint32_t i = 0; i < n && D->post.nundist; i++)   // each slot's camera, beside the frame descriptors (the model describes the detected image)
    D->h_ucams[i] = undistort_cam(D->undist_models[UD_MODEL_OF_SLOT(i, D->post.nundist)]);   // (tools_hooks.h: i % ncams)
  if (D->pending_hash_grow) {   // the pair table of the previous submission was crowded: grow it now (its buffers are dead)
    D->pending_hash_grow = false;
    const GrowPlan g = plan_pending_hash(caps_of(D), D->grow);
    if (g.family != GROW_NONE && !regrow(D, g)) {
      if (D->unusable) return AMDAT_OUT_OF_MEMORY;
      give_up(D->grow, g.family);
    }
  }
  if (D->tables_dirty) { const int crc = clear_hash_tables(D); if (crc) return crc; }
  D->tables_dirty = true;
  const int rc = launch_once(D, n, ostride, s, fmt);
  if (rc) return rc;
  D->inflight.active = true; D->inflight.n = n; D->inflight.ostride = ostride; D->inflight.stream = s;
  return AMDAT_SUCCESS;
}

static int end_batch(amdAprilTagsDetector_st* D) {
  if (!D->inflight.active) return AMDAT_INVALID_ARGUMENT;
  DeviceGuard guard(D->device);
  if (!guard.ok) return AMDAT_HIP_ERROR;
  const uint32_t n = D->inflight.n, ostride = D->inflight.ostride;
  const hipStream_t s = D->inflight.stream;
  D->inflight.active = false;
  for (;;) {
    const int rc = finish_once(D, s);
    if (rc) return rc;
    D->tables_dirty = false;   // ran to its end: k_cluster_select left the pair table empty
    // an overflowed capacity that follows the content grows (growth.h) and the submission runs again; an unusable handle stops
    const GrowPlan g = grow_round(D->h_counters, n, caps_of(D), D->grow, [&](const GrowPlan& p) { return regrow(D, p) || D->unusable; });
    if (D->unusable) return AMDAT_OUT_OF_MEMORY;
    if (g.cands_as_quads) report_cands_as_quads(D->h_counters, n);
    if (g.family == GROW_NONE) { D->pending_hash_grow = g.hash_next; return AMDAT_SUCCESS; }
    if (D->tables_dirty) { const int crc = clear_hash_tables(D); if (crc) return crc; }
    D->tables_dirty = true;
    const int lrc = launch_once(D, n, ostride, s, D->launched_fmt);
    if (lrc) return lrc;
  }
}

static int run_batch(amdAprilTagsDetector_st* D, uint32_t n, const amdAprilTagsImageInput_t* images,
                     const amdAprilTagsCameraIntrinsics_t* intr, uint32_t ostride, hipStream_t s, uint32_t fmt = AMDAT_ENC_MONO8) {
  const int rc = begin_batch(D, n, images, intr, ostride, s, fmt);
  return rc ? rc : end_batch(D);
}

// copies the finished submission's records out of the pinned buffers
static void copy_out_ex(amdAprilTagsDetector_st* D, uint32_t n, uint32_t ostride, uint32_t max_dets, amdAprilTagsDetectionEx_t* dets_out, uint32_t* num_dets) {
  for (uint32_t f = 0; f < n; f++) {
    uint32_t k = D->h_counters[f].nout;
    if (k > ostride) k = ostride;
    num_dets[f] = k;
    memcpy(dets_out + (size_t)f * max_dets, D->h_out + (size_t)f * ostride, (size_t)k * sizeof(DetRec));
  }
}

int amdAprilTagsDetectBatchColorEx(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsImageInput_t* images, amdAprilTagsEncoding encoding,
                                   const amdAprilTagsCameraIntrinsics_t* per_frame_intrinsics, amdAprilTagsDetectionEx_t* dets_out,
                                   uint32_t* num_dets, uint32_t max_dets, amdAprilTagsStream stream) {
  if (!handle || !dets_out || !num_dets || max_dets == 0) return AMDAT_INVALID_ARGUMENT;
  int rc = check_images(handle, n, images, (uint32_t)encoding, !handle->resize_sizes.empty());
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : handle->own_stream;
  uint32_t ostride = max_dets < handle->P.dcap ? max_dets : handle->P.dcap;
  rc = run_batch(handle, n, images, per_frame_intrinsics, ostride, s, (uint32_t)encoding);
  if (rc) return rc;
  copy_out_ex(handle, n, ostride, max_dets, dets_out, num_dets);
  return AMDAT_SUCCESS;
}

int amdAprilTagsDetectBatchEx(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsImageInput_t* images,
                              const amdAprilTagsCameraIntrinsics_t* per_frame_intrinsics, amdAprilTagsDetectionEx_t* dets_out,
                              uint32_t* num_dets, uint32_t max_dets, amdAprilTagsStream stream) {
  return amdAprilTagsDetectBatchColorEx(handle, n, images, AMDAT_ENC_MONO8, per_frame_intrinsics, dets_out, num_dets, max_dets, stream);
}

static void to_public(const DetRec& d, uint16_t family_enum, uint32_t corner_convention, amdAprilTagsID_t* o) {
  memset(o, 0, sizeof(*o));
  o->id = (uint16_t)d.id;
  // library-native corner order = message order = AprilRobotics p[3-i]; AMDAT_CORNERS_ROTATED_180 starts two corners later
  // and turns the tag frame about its normal: R * Rz(pi) = R with its first two columns negated
  const int turn = corner_convention == AMDAT_CORNERS_ROTATED_180 ? 2 : 0;
  const double sgn = turn ? -1.0 : 1.0;
  for (int i = 0; i < 4; i++) { o->corners[i].x = (float)d.p[(3 - i + turn) & 3][0]; o->corners[i].y = (float)d.p[(3 - i + turn) & 3][1]; }
  o->hamming_error = (uint16_t)d.hamming;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) o->orientation[c * 3 + r] = (float)(c < 2 ? sgn * d.R[r * 3 + c] : d.R[r * 3 + c]);  // column-major
  for (int i = 0; i < 3; i++) o->translation[i] = (float)d.t[i];
  o->family = family_enum;
  o->decision_margin = d.decision_margin;
  o->center.x = (float)d.c[0];
  o->center.y = (float)d.c[1];
}

static void copy_out_public(amdAprilTagsDetector_st* D, uint32_t n, uint32_t ostride, uint32_t max_tags, amdAprilTagsID_t* tags_out, uint32_t* num_tags) {
  for (uint32_t f = 0; f < n; f++) {
    uint32_t k = D->h_counters[f].nout;
    if (k > ostride) k = ostride;
    num_tags[f] = k;
    for (uint32_t i = 0; i < k; i++) {
      const DetRec& d = D->h_out[(size_t)f * ostride + i];
      to_public(d, (uint16_t)D->cfg.families[d.family], D->cfg.corner_convention, &tags_out[(size_t)f * max_tags + i]);
    }
  }
}

int amdAprilTagsDetectBatchColor(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsImageInput_t* images, amdAprilTagsEncoding encoding,
                                 const amdAprilTagsCameraIntrinsics_t* per_frame_intrinsics, amdAprilTagsID_t* tags_out,
                                 uint32_t* num_tags, uint32_t max_tags, amdAprilTagsStream stream) {
  if (!handle || !tags_out || !num_tags || max_tags == 0) return AMDAT_INVALID_ARGUMENT;
  int rc = check_images(handle, n, images, (uint32_t)encoding, !handle->resize_sizes.empty());
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : handle->own_stream;
  uint32_t ostride = max_tags < handle->P.dcap ? max_tags : handle->P.dcap;
  rc = run_batch(handle, n, images, per_frame_intrinsics, ostride, s, (uint32_t)encoding);
  if (rc) return rc;
  copy_out_public(handle, n, ostride, max_tags, tags_out, num_tags);
  return AMDAT_SUCCESS;
}

int amdAprilTagsDetectBatch(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsImageInput_t* images,
                            const amdAprilTagsCameraIntrinsics_t* per_frame_intrinsics, amdAprilTagsID_t* tags_out,
                            uint32_t* num_tags, uint32_t max_tags, amdAprilTagsStream stream) {
  return amdAprilTagsDetectBatchColor(handle, n, images, AMDAT_ENC_MONO8, per_frame_intrinsics, tags_out, num_tags, max_tags, stream);
}

int amdAprilTagsDetectColor(amdAprilTagsHandle handle, const amdAprilTagsImageInput_t* img_input, amdAprilTagsEncoding encoding,
                            amdAprilTagsID_t* tags_out, uint32_t* num_tags, uint32_t max_tags, amdAprilTagsStream stream) {
  // The cuAprilTagsDetect-shaped call keeps to the reference's encoding table, as it always has: the raw formats go through the batched
  // forms (n = 1 for one frame).
  if ((uint32_t)encoding > AMDAT_ENC_BGRA8) return AMDAT_UNSUPPORTED;
  return amdAprilTagsDetectBatchColor(handle, 1, img_input, encoding, nullptr, tags_out, num_tags, max_tags, stream);
}

// ---- the same submission in two halves: enqueue, then wait -------------------------------------------------------------
// amdAprilTagsSubmitBatch returns as soon as the submission is enqueued on the stream; the host is free -- to copy the NEXT
// batch's frames to the device on a stream of its own, to serve other handles -- until amdAprilTagsWaitBatch[Ex] blocks for
// the results.  One submission per handle may be in flight; the images (and their device buffers) must stay valid until the
// wait returns.  Submit + Wait gives exactly what the blocking call gives (the blocking call IS the two, back to back).
int amdAprilTagsSubmitBatchColor(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsImageInput_t* images, amdAprilTagsEncoding encoding,
                                 const amdAprilTagsCameraIntrinsics_t* per_frame_intrinsics, uint32_t max_tags, amdAprilTagsStream stream) {
  if (!handle || max_tags == 0) return AMDAT_INVALID_ARGUMENT;
  int rc = check_images(handle, n, images, (uint32_t)encoding, !handle->resize_sizes.empty());
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : handle->own_stream;
  const uint32_t ostride = max_tags < handle->P.dcap ? max_tags : handle->P.dcap;
  rc = begin_batch(handle, n, images, per_frame_intrinsics, ostride, s, (uint32_t)encoding);
  if (rc) return rc;
  handle->inflight.max_out = max_tags;
  return AMDAT_SUCCESS;
}

int amdAprilTagsSubmitBatch(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsImageInput_t* images,
                            const amdAprilTagsCameraIntrinsics_t* per_frame_intrinsics, uint32_t max_tags, amdAprilTagsStream stream) {
  return amdAprilTagsSubmitBatchColor(handle, n, images, AMDAT_ENC_MONO8, per_frame_intrinsics, max_tags, stream);
}

int amdAprilTagsWaitBatch(amdAprilTagsHandle handle, amdAprilTagsID_t* tags_out, uint32_t* num_tags) {
  if (!handle || !tags_out || !num_tags || !handle->inflight.active) return AMDAT_INVALID_ARGUMENT;
  const uint32_t n = handle->inflight.n, ostride = handle->inflight.ostride, max_tags = handle->inflight.max_out;
  const int rc = end_batch(handle);
  if (rc) return rc;
  copy_out_public(handle, n, ostride, max_tags, tags_out, num_tags);
  return AMDAT_SUCCESS;
}

int amdAprilTagsWaitBatchEx(amdAprilTagsHandle handle, amdAprilTagsDetectionEx_t* dets_out, uint32_t* num_dets) {
  if (!handle || !dets_out || !num_dets || !handle->inflight.active) return AMDAT_INVALID_ARGUMENT;
  const uint32_t n = handle->inflight.n, ostride = handle->inflight.ostride, max_dets = handle->inflight.max_out;
  const int rc = end_batch(handle);
  if (rc) return rc;
  copy_out_ex(handle, n, ostride, max_dets, dets_out, num_dets);
  return AMDAT_SUCCESS;
}

int amdAprilTagsDetect(amdAprilTagsHandle handle, const amdAprilTagsImageInput_t* img_input, amdAprilTagsID_t* tags_out,
                       uint32_t* num_tags, uint32_t max_tags, amdAprilTagsStream stream) {
  return amdAprilTagsDetectBatch(handle, 1, img_input, nullptr, tags_out, num_tags, max_tags, stream);
}

int amdAprilTagsSetFrameSkews(amdAprilTagsHandle handle, uint32_t n, const float* skews) {
  if (!handle || n > handle->cfg.max_batch || (n && !skews) || handle->inflight.active) return AMDAT_INVALID_ARGUMENT;
  handle->frame_skew.assign(skews, skews + n);
  return AMDAT_SUCCESS;
}

// The shift of 16-bit samples (raw_formats.h): host state that travels with the descriptors, so no graph is retired.
int amdAprilTagsSetRawShift(amdAprilTagsHandle handle, uint32_t shift) {
  if (!handle || shift > RAW_MAX_SHIFT || handle->inflight.active) return AMDAT_INVALID_ARGUMENT;
  handle->raw_shift = shift;
  return AMDAT_SUCCESS;
}

int amdAprilTagsGetFrameFlags(amdAprilTagsHandle handle, uint32_t* flags, uint32_t n) {
  if (!handle || !flags || n > handle->last.n || handle->inflight.active) return AMDAT_INVALID_ARGUMENT;
  for (uint32_t i = 0; i < n; i++) flags[i] = handle->h_counters[i].flags;
  return AMDAT_SUCCESS;
}

int amdAprilTagsThresholdOnly(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsImageInput_t* images,
                              amdAprilTagsStream stream) {
  return amdAprilTagsThresholdOnlyColor(handle, n, images, AMDAT_ENC_MONO8, stream);
}

int amdAprilTagsThresholdOnlyColor(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsImageInput_t* images, amdAprilTagsEncoding encoding,
                                   amdAprilTagsStream stream) {
  if (!handle || handle->inflight.active) return AMDAT_INVALID_ARGUMENT;
  const uint32_t fmt = (uint32_t)encoding;
  if (raw_is_raw(fmt)) return AMDAT_UNSUPPORTED;   // (the roofline launch: it never runs a front step)
  int rc = check_images(handle, n, images, fmt);
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : handle->own_stream;
  DeviceGuard guard(handle->device);
  if (!guard.ok) return AMDAT_HIP_ERROR;
  rc = ensure_colour_plane(handle, fmt);
  if (rc) return rc;
  fill_frames(handle, n, images, nullptr, fmt);
  handle->last = {};   // (never runs the front stage or the stages behind k_reconcile)
  handle->last.n = n;
  HIP_TRY(hipMemcpyAsync(handle->d_frames, handle->h_frames, n * sizeof(FrameDesc), hipMemcpyHostToDevice, s));
  if (handle->profiling) hipEventRecord(handle->ev[1], s);
  { DetParams P0 = handle->P; P0.frame0 = 0; launch_threshold(handle, P0, n, s, fmt); }
  if (handle->profiling) hipEventRecord(handle->ev[2], s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  if (handle->profiling) {
    memset(handle->stage_ms, 0, sizeof(handle->stage_ms));
    hipEventElapsedTime(&handle->stage_ms[1], handle->ev[1], handle->ev[2]);
  }
  return AMDAT_SUCCESS;
}

int amdAprilTagsConvertToMono8(const void* src_dev, size_t src_pitch, const char* encoding, uint32_t width, uint32_t height,
                               uint8_t* dst_dev, size_t dst_pitch, amdAprilTagsStream stream) {
  if (!src_dev || !dst_dev || !encoding || width == 0 || height == 0) return AMDAT_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  const uint8_t* src = (const uint8_t*)src_dev;
  dim3 grid((width + 1023) / 1024, height), block(256);
  if (!strcmp(encoding, "mono8")) {
    HIP_TRY(hipMemcpy2DAsync(dst_dev, dst_pitch, src_dev, src_pitch, width, height, hipMemcpyDeviceToDevice, s));
  } else if (!strcmp(encoding, "rgb8")) {
    hipLaunchKernelGGL((k_to_mono8<3, 0, 2>), grid, block, 0, s, src, src_pitch, dst_dev, dst_pitch, width, height);
  } else if (!strcmp(encoding, "bgr8")) {
    hipLaunchKernelGGL((k_to_mono8<3, 2, 0>), grid, block, 0, s, src, src_pitch, dst_dev, dst_pitch, width, height);
  } else if (!strcmp(encoding, "rgba8")) {
    hipLaunchKernelGGL((k_to_mono8<4, 0, 2>), grid, block, 0, s, src, src_pitch, dst_dev, dst_pitch, width, height);
  } else if (!strcmp(encoding, "bgra8")) {
    hipLaunchKernelGGL((k_to_mono8<4, 2, 0>), grid, block, 0, s, src, src_pitch, dst_dev, dst_pitch, width, height);
  } else if (raw_is_raw((uint32_t)amdAprilTagsEncodingFromName(encoding))) {   // (the raw formats at the default shift)
    return amdAprilTagsConvertRawToMono8(src_dev, src_pitch, (amdAprilTagsEncoding)amdAprilTagsEncodingFromName(encoding), RAW_MAX_SHIFT, width, height,
                                         dst_dev, dst_pitch, stream);
  } else {
    return AMDAT_UNSUPPORTED;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  return AMDAT_SUCCESS;
}

// The stand-alone form of the raw conversion: the device function of k_raw_to_mono8_frames for one frame, into a caller's plane at any
// address and pitch (the bytes beyond `width` of a row are left as they are).
int amdAprilTagsConvertRawToMono8(const void* src_dev, size_t src_pitch, amdAprilTagsEncoding encoding, uint32_t shift, uint32_t width, uint32_t height,
                                  uint8_t* dst_dev, size_t dst_pitch, amdAprilTagsStream stream) {
  const uint32_t fmt = (uint32_t)encoding;
  if (!src_dev || !dst_dev || width == 0 || height == 0 || shift > RAW_MAX_SHIFT || dst_pitch < width) return AMDAT_INVALID_ARGUMENT;
  if (!raw_is_raw(fmt)) return AMDAT_UNSUPPORTED;
  if (width > 16384 || height > 16384 || (raw_is_bayer(fmt) && (width < 2 || height < 2))) return AMDAT_SIZE_MISMATCH;
  if (src_pitch < (size_t)width * raw_bytes_per_sample(fmt) || src_pitch >= (1u << 24) || dst_pitch >= (1u << 24)) return AMDAT_INVALID_ARGUMENT;
  if (raw_is_16(fmt) && (((uintptr_t)src_dev | src_pitch) & 1u)) return AMDAT_INVALID_ARGUMENT;
  RawDesc d;
  d.src = (const uint8_t*)src_dev; d.dst = dst_dev;
  d.src_pitch = (uint32_t)src_pitch; d.dst_pitch = (uint32_t)dst_pitch;
  d.enc = fmt; d.shift = shift;
  d.w = (int32_t)width; d.h = (int32_t)height;
  d.store = (((uintptr_t)dst_dev | dst_pitch) & 3u) ? RAW_STORE_BYTES : RAW_STORE_DWORD; d.pad = 0;
  hipStream_t s = (hipStream_t)stream;
  const dim3 g((width + RAW_BW - 1) / RAW_BW, (height + RAW_BH - 1) / RAW_BH);
  switch (raw_kind(fmt)) {
    case RAW_KIND_BAYER8: hipLaunchKernelGGL(k_raw_to_mono8<RAW_KIND_BAYER8>, g, dim3(256), 0, s, d); break;
    case RAW_KIND_MONO16: hipLaunchKernelGGL(k_raw_to_mono8<RAW_KIND_MONO16>, g, dim3(256), 0, s, d); break;
    default: hipLaunchKernelGGL(k_raw_to_mono8<RAW_KIND_BAYER16>, g, dim3(256), 0, s, d); break;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  return AMDAT_SUCCESS;
}

int amdAprilTagsResizeMono8(const uint8_t* src_dev, size_t src_pitch, uint32_t sw, uint32_t sh, uint8_t* dst_dev, size_t dst_pitch,
                            uint32_t dw, uint32_t dh, amdAprilTagsStream stream) {
  if (!src_dev || !dst_dev || sw == 0 || sh == 0 || dw == 0 || dh == 0 || src_pitch < sw || dst_pitch < dw) return AMDAT_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_resize_mono8, dim3((dw + 63) / 64, (dh + 3) / 4), dim3(256), 0, s, src_dev, src_pitch, (int)sw, (int)sh, dst_dev,
                     dst_pitch, (int)dw, (int)dh);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  return AMDAT_SUCCESS;
}

int amdAprilTagsRectifyMono8(const uint8_t* src_dev, size_t src_pitch, uint8_t* dst_dev, size_t dst_pitch, uint32_t width,
                             uint32_t height, const double* K9, const double* D5, const double* Knew9, amdAprilTagsStream stream) {
  if (!src_dev || !dst_dev || !K9 || !D5 || !Knew9 || width == 0 || height == 0 || src_pitch < width || dst_pitch < width)
    return AMDAT_INVALID_ARGUMENT;
  RectifyParams R = {K9[0], K9[4], K9[2], K9[5], D5[0], D5[1], D5[2], D5[3], D5[4], Knew9[0], Knew9[4], Knew9[2], Knew9[5]};
  if (R.nfx == 0.0 || R.nfy == 0.0) return AMDAT_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rectify_mono8, dim3((width + 63) / 64, (height + 3) / 4), dim3(256), 0, s, src_dev, src_pitch, dst_dev, dst_pitch,
                     (int)width, (int)height, R);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  return AMDAT_SUCCESS;
}

int amdAprilTagsRectifyMono8Ex(const uint8_t* src_dev, size_t src_pitch, uint8_t* dst_dev, size_t dst_pitch, uint32_t width,
                               uint32_t height, const amdAprilTagsCameraModelEx_t* cam, amdAprilTagsStream stream) {
  if (!src_dev || !dst_dev || !cam || width == 0 || height == 0 || src_pitch < width || dst_pitch < width || !camera_model_ok(*cam))
    return AMDAT_INVALID_ARGUMENT;
  RectifyParams R;
  CamGeneral G;
  camera_model_params(*cam, R, G);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((width + 63) / 64, (height + 3) / 4);
  if (G.general)
    hipLaunchKernelGGL(k_rectify_mono8_ex, grid, dim3(256), 0, s, src_dev, src_pitch, dst_dev, dst_pitch, (int)width, (int)height, R, G);
  else
    hipLaunchKernelGGL(k_rectify_mono8, grid, dim3(256), 0, s, src_dev, src_pitch, dst_dev, dst_pitch, (int)width, (int)height, R);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  return AMDAT_SUCCESS;
}

int amdAprilTagsDeviceAlloc(void** dev_ptr, size_t bytes) {
  if (!dev_ptr || bytes == 0) return AMDAT_INVALID_ARGUMENT;
  return hipMalloc(dev_ptr, bytes) == hipSuccess ? AMDAT_SUCCESS : AMDAT_OUT_OF_MEMORY;
}
int amdAprilTagsDeviceFree(void* dev_ptr) {
  if (!dev_ptr) return AMDAT_INVALID_ARGUMENT;
  return hipFree(dev_ptr) == hipSuccess ? AMDAT_SUCCESS : AMDAT_HIP_ERROR;
}
int amdAprilTagsCopyToDevice(void* dst_dev, const void* src_host, size_t bytes, amdAprilTagsStream stream) {
  if (!dst_dev || !src_host) return AMDAT_INVALID_ARGUMENT;
  HIP_TRY(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return AMDAT_SUCCESS;
}

// enqueue-only copy + stream helpers for hosts that do not link the HIP runtime (the node shell): the copy is ordered on `stream`
// ahead of the detection the host enqueues on the same stream, and the detection's own wait covers it -- no second host wait
int amdAprilTagsCopyToDeviceAsync(void* dst_dev, const void* src_host, size_t bytes, amdAprilTagsStream stream) {
  if (!dst_dev || !src_host || !stream) return AMDAT_INVALID_ARGUMENT;
  HIP_TRY(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return AMDAT_SUCCESS;
}
int amdAprilTagsStreamCreate(amdAprilTagsStream* stream) {
  if (!stream) return AMDAT_INVALID_ARGUMENT;
  hipStream_t s = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *stream = (amdAprilTagsStream)s;
  return AMDAT_SUCCESS;
}
int amdAprilTagsStreamDestroy(amdAprilTagsStream stream) {
  if (!stream) return AMDAT_INVALID_ARGUMENT;
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  HIP_TRY(hipStreamDestroy((hipStream_t)stream));
  return AMDAT_SUCCESS;
}

int amdAprilTagsDebugCopy(amdAprilTagsHandle handle, uint32_t frame, amdAprilTagsDebugBuffer what, void* host_dst,
                          size_t capacity, size_t* bytes) {
  if (!handle || !bytes || frame >= handle->last.n || handle->inflight.active) return AMDAT_INVALID_ARGUMENT;
  const DetParams& P = handle->P;
  DeviceGuard guard(handle->device);
  if (!guard.ok) return AMDAT_HIP_ERROR;
  HIP_TRY(hipDeviceSynchronize());
  const FrameCounters& fc = handle->h_counters[frame];
  // the frame's own working size (the descriptor block still holds the last submission): dense fW x fH planes; slots are the handle's
  const int fW = handle->h_frames[frame].W, fH = handle->h_frames[frame].H;
  const size_t npx = (size_t)fW * fH, slot_px = (size_t)P.W * P.H;
  const void* src = nullptr;
  size_t sz = 0;
  std::vector<uint8_t> tmp;
  switch (what) {
    case AMDAT_DBG_GRAY:
    case AMDAT_DBG_THRESH: {
      // de-pitch rows on the host
      const uint8_t* base = nullptr;
      size_t pitch = P.WS;
      if (what == AMDAT_DBG_THRESH) base = handle->d_thr + (size_t)frame * P.H * P.WS;
      else if (P.decimate > 1) base = handle->d_gray + (size_t)frame * P.H * P.WS;
      else { base = handle->h_frames[frame].img; pitch = handle->h_frames[frame].pitch; }
      tmp.resize(npx);
      HIP_TRY(hipMemcpy2D(tmp.data(), fW, base, pitch, fW, fH, hipMemcpyDeviceToHost));
      *bytes = npx;
      if (host_dst) memcpy(host_dst, tmp.data(), npx < capacity ? npx : capacity);
      return AMDAT_SUCCESS;
    }
    case AMDAT_DBG_RECTIFIED:
    case AMDAT_DBG_RESIZED: {   // DW x DH dense: the frame's slot of the front plane, where the last submission formed that plane
      if (what == AMDAT_DBG_RESIZED ? handle->resize_sizes.empty() || !handle->last.resized : handle->rect_models.empty() || !handle->last.rectified)
        return AMDAT_INVALID_ARGUMENT;
      const FrontDesc& f = handle->h_front[frame];
      const size_t n0 = (size_t)f.DW * f.DH;
      tmp.resize(n0);
      HIP_TRY(hipMemcpy2D(tmp.data(), f.DW, f.dst, f.dst_pitch, f.DW, f.DH, hipMemcpyDeviceToHost));
      *bytes = n0;
      if (host_dst) memcpy(host_dst, tmp.data(), n0 < capacity ? n0 : capacity);
      return AMDAT_SUCCESS;
    }
    case AMDAT_DBG_RAW_GRAY: {   // w x h dense at the source size: the frame's slot of d_raw, where the last submission converted into it
      if (!handle->last.raw) return AMDAT_INVALID_ARGUMENT;
      const RawDesc& r = handle->h_rawdesc[frame];
      const size_t n0 = (size_t)r.w * r.h;
      tmp.resize(n0);
      HIP_TRY(hipMemcpy2D(tmp.data(), r.w, r.dst, r.dst_pitch, r.w, r.h, hipMemcpyDeviceToHost));
      *bytes = n0;
      if (host_dst) memcpy(host_dst, tmp.data(), n0 < capacity ? n0 : capacity);
      return AMDAT_SUCCESS;
    }
    case AMDAT_DBG_LABEL: {
      DetParams Pf = P;
      Pf.frame0 = (int)frame;
      hipLaunchKernelGGL(k_cc_flatten, dim3((unsigned)((npx + 255) / 256), 1, 1), dim3(256), 0, 0, handle->d_label, npx, Pf);
      HIP_TRY(hipDeviceSynchronize());
      src = handle->d_label + (size_t)frame * slot_px; sz = npx * 4;
      break;
    }
    case AMDAT_DBG_CSIZE: src = handle->d_csize + (size_t)frame * slot_px; sz = npx * 4; break;
    case AMDAT_DBG_CLUSTERS:
      src = handle->d_clusters + (size_t)frame * P.ccap;
      sz = (size_t)(fc.nclusters < P.ccap ? fc.nclusters : P.ccap) * sizeof(ClusterRec);
      break;
    case AMDAT_DBG_POINTS:
      src = handle->d_pts + (size_t)frame * P.pcap;
      sz = (size_t)(fc.npoints_kept < P.pcap ? fc.npoints_kept : P.pcap) * 4;
      break;
    case AMDAT_DBG_QUADS:
      src = handle->d_quads + (size_t)frame * P.qcap;
      sz = (size_t)(fc.nquads < P.qcap ? fc.nquads : P.qcap) * sizeof(QuadRec);
      break;
    case AMDAT_DBG_DETS:   // as k_decode_wave wrote them: atomic slots, R and t zero (ndets counts every attempt, the list holds dcap)
      src = handle->d_dets + (size_t)frame * P.dcap;
      sz = (size_t)(fc.ndets < P.dcap ? fc.ndets : P.dcap) * sizeof(DetRec);
      break;
    case AMDAT_DBG_FQPROF:
      src = handle->d_fqprof; sz = (64 + 8) * 8;
      break;
    case AMDAT_DBG_COUNTS: {
      uint32_t c[8] = {fc.npoints_raw, fc.nclusters, fc.npoints_kept, fc.nquads, fc.ndets, fc.flags, (uint32_t)fW, (uint32_t)fH};
      *bytes = sizeof(c);
      if (host_dst) memcpy(host_dst, c, sizeof(c) < capacity ? sizeof(c) : capacity);
      return AMDAT_SUCCESS;
    }
    default: return AMDAT_INVALID_ARGUMENT;
  }
  *bytes = sz;
  if (host_dst && sz) HIP_TRY(hipMemcpy(host_dst, src, sz < capacity ? sz : capacity, hipMemcpyDeviceToHost));
  return AMDAT_SUCCESS;
}

// One stage alone on batch slot 0, for the two entry points below.  The slot's descriptor carries the handle's intrinsics and a fresh
// sequence number, its counters are `fc`; `enqueue(s, P)` uploads what else the stage reads and launches it; `stamped(seq)` says
// whether its results have arrived, asked after the stream wait and once more after a device-wide one.  Nothing of the last
// submission can be inspected afterwards (its slot 0 is overwritten): the snapshot is empty, last.n 0, until the next one, whose
// prologue rewrites descriptors and counters anyway.
extern "C++" {
template <class Enqueue, class Stamped>
static int debug_slot0(amdAprilTagsDetector_st* D, const FrameCounters& fc, Enqueue enqueue, Stamped stamped) {
  const hipStream_t s = D->own_stream;
  HIP_TRY(hipDeviceSynchronize());
  D->last = {};
  FrameDesc fd;
  memset(&fd, 0, sizeof(fd));
  fd.fx = (double)D->cfg.intrinsics.fx; fd.fy = (double)D->cfg.intrinsics.fy;
  fd.cx = (double)D->cfg.intrinsics.cx; fd.cy = (double)D->cfg.intrinsics.cy;
  fd.skew = (double)(D->frame_skew.empty() ? D->cfg.skew : D->frame_skew[0]);
  fd.seq = ++D->seq;
  HIP_TRY(hipMemcpyAsync(D->d_frames, &fd, sizeof(fd), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(D->d_counters, &fc, sizeof(fc), hipMemcpyHostToDevice, s));
  DetParams P = D->P;
  P.frame0 = 0;
  { const int rc = enqueue(s, P); if (rc) return rc; }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));   // (the pageable sources above are read before this returns)
  if (!stamped(fd.seq)) {
    HIP_TRY(hipDeviceSynchronize());
    if (!stamped(fd.seq)) return AMDAT_HIP_ERROR;
  }
  return AMDAT_SUCCESS;
}
}  // extern "C++"

// k_reconcile alone, on records the caller chooses: they go into batch slot 0's record list with that slot's ndets, and the kept
// records come back through the pinned buffer as after a submission.
int amdAprilTagsDebugReconcile(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsDetectionEx_t* records_in,
                               amdAprilTagsDetectionEx_t* records_out, uint32_t capacity, uint32_t* nout) {
  if (!handle || !nout || handle->inflight.active || (n && !records_in) || (capacity && !records_out)) return AMDAT_INVALID_ARGUMENT;
  if (n > handle->P.dcap) return AMDAT_INVALID_ARGUMENT;
  if (handle->unusable) return AMDAT_OUT_OF_MEMORY;
  amdAprilTagsDetector_st* D = handle;
  DeviceGuard guard(D->device);
  if (!guard.ok) return AMDAT_HIP_ERROR;
  FrameCounters fc;
  memset(&fc, 0, sizeof(fc));
  fc.ndets = n;
  const int rc = debug_slot0(D, fc,
      [&](hipStream_t s, const DetParams& P) -> int {
        if (n) HIP_TRY(hipMemcpyAsync(D->d_dets, records_in, (size_t)n * sizeof(DetRec), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_reconcile, dim3(1), dim3(64), 0, s, D->d_frames, D->d_dets, D->d_counters, D->d_order, D->h_out, P.dcap,
                           D->h_counters, P, (const void*)D->d_tag_table.p);
        return AMDAT_SUCCESS;
      },
      [&](uint32_t seq) { return static_cast<volatile FrameCounters*>(D->h_counters)[0].seq == seq; });
  if (rc) return rc;
  const uint32_t nk = D->h_counters[0].nout;
  *nout = nk;
  const uint32_t k = nk < capacity ? nk : capacity;
  if (k) memcpy(records_out, D->h_out, (size_t)k * sizeof(DetRec));
  return AMDAT_SUCCESS;
}

// k_undistort_records alone, on records the caller chooses: they become batch slot 0's kept records in the order given (the order list
// is the identity), under `cam`.
int amdAprilTagsDebugUndistort(amdAprilTagsHandle handle, uint32_t n, const amdAprilTagsDetectionEx_t* records_in,
                               const amdAprilTagsCameraModelEx_t* cam, amdAprilTagsUndistortedDetection_t* out,
                               amdAprilTagsDetectionEx_t* twins_out) {
  if (!handle || !cam || handle->inflight.active || (n && !records_in) || !camera_model_ok(*cam)) return AMDAT_INVALID_ARGUMENT;
  if (n > handle->P.dcap) return AMDAT_INVALID_ARGUMENT;
  if (handle->unusable) return AMDAT_OUT_OF_MEMORY;
  amdAprilTagsDetector_st* D = handle;
  DeviceGuard guard(D->device);
  if (!guard.ok) return AMDAT_HIP_ERROR;
  { const int rc = ensure_undistort_buffers(D); if (rc) return rc; }
  FrameCounters fc;
  memset(&fc, 0, sizeof(fc));
  fc.ndets = n; fc.nout = n;
  const UndistortCam uc = undistort_cam(*cam);
  std::vector<uint16_t> ident(n);
  for (uint32_t i = 0; i < n; i++) ident[i] = (uint16_t)i;
  const int rc = debug_slot0(D, fc,
      [&](hipStream_t s, const DetParams& P) -> int {
        HIP_TRY(hipMemcpyAsync(D->d_ucams, &uc, sizeof(uc), hipMemcpyHostToDevice, s));
        if (n) {
          HIP_TRY(hipMemcpyAsync(D->d_dets, records_in, (size_t)n * sizeof(DetRec), hipMemcpyHostToDevice, s));
          HIP_TRY(hipMemcpyAsync(D->d_order, ident.data(), (size_t)n * sizeof(uint16_t), hipMemcpyHostToDevice, s));
        }
        hipLaunchKernelGGL(k_undistort_records, dim3(1, UD_WAVES_PER_FRAME), dim3(64), 0, s, D->d_frames, D->d_dets, D->d_counters, D->d_order,
                           D->d_ucams, D->d_dets_u, D->h_udets, P.dcap, P, (const void*)D->d_tag_table.p);
        return AMDAT_SUCCESS;
      },
      [&](uint32_t seq) {
        for (uint32_t i = 0; i < n; i++)
          if (static_cast<volatile UndistortRec*>(D->h_udets)[i].seq != seq) return false;
        return true;
      });
  if (rc) return rc;
  if (out) for (uint32_t i = 0; i < n; i++) out[i] = D->h_udets[i].det;
  if (twins_out && n) HIP_TRY(hipMemcpy(twins_out, D->d_dets_u, (size_t)n * sizeof(DetRec), hipMemcpyDeviceToHost));
  return AMDAT_SUCCESS;
}

#include "tools_timeline.h"   // debug entry points of the -DAMDAT_FQ_TIMELINE tools build; empty in the product build

int amdAprilTagsDebugMath(int op, uint32_t n, const double* a, const double* b, double* out) {
  if (!a || !b || !out || n == 0) return AMDAT_INVALID_ARGUMENT;
  double *da = nullptr, *db = nullptr, *dout = nullptr;
  int rc = AMDAT_HIP_ERROR;
  if (hipMalloc((void**)&da, n * 8) == hipSuccess && hipMalloc((void**)&db, n * 8) == hipSuccess &&
      hipMalloc((void**)&dout, n * 8) == hipSuccess && hipMemcpy(da, a, n * 8, hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(db, b, n * 8, hipMemcpyHostToDevice) == hipSuccess) {
    hipLaunchKernelGGL(k_debug_math, dim3((n + 255) / 256), dim3(256), 0, 0, op, n, da, db, dout);
    if (hipGetLastError() == hipSuccess && hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost) == hipSuccess) rc = AMDAT_SUCCESS;
  }
  hipFree(da); hipFree(db); hipFree(dout);
  return rc;
}

}  // extern "C"
