// node_shell.cpp -- implementation of include/apriltag_node_shell.hpp: the reference node's host logic
// (src/apriltag_node.cpp:389-623) over the C ABI of libapriltag_amd.so.  Built into libapriltag_node.so;
// the detector library is bound at run time (dlopen next to this file's .so), so this translation unit
// needs neither HIP headers nor ROS.
#include "../../include/apriltag_node_shell.hpp"

#include <dlfcn.h>

#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <sstream>
#include <stdexcept>

#include "../../include/apriltag_amd.h"

namespace amd {
namespace isaac_ros {
namespace apriltag {

namespace {

// Entry points of libapriltag_amd.so used by the shell.
struct DetectorApi {
  void* lib = nullptr;
  decltype(&amdCreateAprilTagsDetectorEx) create_ex = nullptr;
  decltype(&amdAprilTagsDefaultConfig) default_config = nullptr;
  decltype(&amdAprilTagsDetect) detect = nullptr;
  decltype(&amdAprilTagsDetectBatch) detect_batch = nullptr;
  decltype(&amdAprilTagsDestroy) destroy = nullptr;
  decltype(&amdAprilTagsFamilyFromName) family_from_name = nullptr;
  decltype(&amdAprilTagsConvertToMono8) to_mono8 = nullptr;
  decltype(&amdAprilTagsDeviceAlloc) dev_alloc = nullptr;
  decltype(&amdAprilTagsDeviceFree) dev_free = nullptr;
  decltype(&amdAprilTagsCopyToDevice) copy_to_device = nullptr;
  decltype(&amdAprilTagsSetFrameSkews) set_frame_skews = nullptr;
  decltype(&amdAprilTagsDetectColor) detect_color = nullptr;
  decltype(&amdAprilTagsDetectBatchColor) detect_batch_color = nullptr;
  decltype(&amdAprilTagsEncodingFromName) encoding_from_name = nullptr;
  decltype(&amdAprilTagsCopyToDeviceAsync) copy_to_device_async = nullptr;
  decltype(&amdAprilTagsStreamCreate) stream_create = nullptr;
  decltype(&amdAprilTagsStreamDestroy) stream_destroy = nullptr;
  decltype(&amdAprilTagsSetQuadSigma) set_quad_sigma = nullptr;
  decltype(&amdAprilTagsSetPerFrameSizes) set_per_frame_sizes = nullptr;
  decltype(&amdAprilTagsSetRectification) set_rectification = nullptr;
  decltype(&amdAprilTagsSetResize) set_resize = nullptr;
  decltype(&amdAprilTagsSetRectificationEx) set_rectification_ex = nullptr;
  decltype(&amdAprilTagsSetBundles) set_bundles = nullptr;
  decltype(&amdAprilTagsGetBundlePoses) get_bundle_poses = nullptr;
  decltype(&amdAprilTagsSetBundlesEx) set_bundles_ex = nullptr;
  decltype(&amdAprilTagsGetBundlePosesEx) get_bundle_poses_ex = nullptr;
  decltype(&amdAprilTagsSetRig) set_rig = nullptr;
  decltype(&amdAprilTagsSetRigSlots) set_rig_slots = nullptr;
  decltype(&amdAprilTagsGetRigBundlePoses) get_rig_bundle_poses = nullptr;
  decltype(&amdAprilTagsSetPoseRefinement) set_pose_refinement = nullptr;
  decltype(&amdAprilTagsGetRefinedPoses) get_refined_poses = nullptr;
  decltype(&amdAprilTagsSetPoseCovariance) set_pose_covariance = nullptr;
  decltype(&amdAprilTagsGetRefinedPoseCovariances) get_refined_pose_covariances = nullptr;
  decltype(&amdAprilTagsGetBundlePoseCovariancesEx) get_bundle_pose_covariances_ex = nullptr;
  decltype(&amdAprilTagsSetCornerUndistortion) set_corner_undistortion = nullptr;
  decltype(&amdAprilTagsGetUndistortedDetections) get_undistorted_detections = nullptr;
  decltype(&amdAprilTagsSetRawShift) set_raw_shift = nullptr;
  decltype(&amdAprilTagsSetTagTable) set_tag_table = nullptr;
};

DetectorApi& api() {
  static DetectorApi a;
  if (a.lib) return a;
  Dl_info info;
  std::string path = "libapriltag_amd.so";
  if (dladdr(reinterpret_cast<void*>(&api), &info) && info.dli_fname) {
    std::string self(info.dli_fname);
    const size_t slash = self.find_last_of('/');
    if (slash != std::string::npos) path = self.substr(0, slash + 1) + "libapriltag_amd.so";
  }
  a.lib = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
  if (!a.lib) throw std::runtime_error(std::string("cannot load libapriltag_amd.so: ") + dlerror());
#define BIND(field, name)                                                        \
  a.field = reinterpret_cast<decltype(a.field)>(dlsym(a.lib, name));             \
  if (!a.field) throw std::runtime_error(std::string("missing symbol ") + name);
  BIND(create_ex, "amdCreateAprilTagsDetectorEx")
  BIND(default_config, "amdAprilTagsDefaultConfig")
  BIND(detect, "amdAprilTagsDetect")
  BIND(detect_batch, "amdAprilTagsDetectBatch")
  BIND(destroy, "amdAprilTagsDestroy")
  BIND(family_from_name, "amdAprilTagsFamilyFromName")
  BIND(to_mono8, "amdAprilTagsConvertToMono8")
  BIND(dev_alloc, "amdAprilTagsDeviceAlloc")
  BIND(dev_free, "amdAprilTagsDeviceFree")
  BIND(copy_to_device, "amdAprilTagsCopyToDevice")
  BIND(set_frame_skews, "amdAprilTagsSetFrameSkews")
  BIND(detect_color, "amdAprilTagsDetectColor")
  BIND(detect_batch_color, "amdAprilTagsDetectBatchColor")
  BIND(encoding_from_name, "amdAprilTagsEncodingFromName")
  BIND(copy_to_device_async, "amdAprilTagsCopyToDeviceAsync")
  BIND(stream_create, "amdAprilTagsStreamCreate")
  BIND(stream_destroy, "amdAprilTagsStreamDestroy")
  BIND(set_quad_sigma, "amdAprilTagsSetQuadSigma")
  BIND(set_per_frame_sizes, "amdAprilTagsSetPerFrameSizes")
  BIND(set_rectification, "amdAprilTagsSetRectification")
  BIND(set_resize, "amdAprilTagsSetResize")
  BIND(set_rectification_ex, "amdAprilTagsSetRectificationEx")
  BIND(set_bundles, "amdAprilTagsSetBundles")
  BIND(get_bundle_poses, "amdAprilTagsGetBundlePoses")
  BIND(set_bundles_ex, "amdAprilTagsSetBundlesEx")
  BIND(get_bundle_poses_ex, "amdAprilTagsGetBundlePosesEx")
  BIND(set_rig, "amdAprilTagsSetRig")
  BIND(set_rig_slots, "amdAprilTagsSetRigSlots")
  BIND(get_rig_bundle_poses, "amdAprilTagsGetRigBundlePoses")
  BIND(set_pose_refinement, "amdAprilTagsSetPoseRefinement")
  BIND(get_refined_poses, "amdAprilTagsGetRefinedPoses")
  BIND(set_pose_covariance, "amdAprilTagsSetPoseCovariance")
  BIND(get_refined_pose_covariances, "amdAprilTagsGetRefinedPoseCovariances")
  BIND(get_bundle_pose_covariances_ex, "amdAprilTagsGetBundlePoseCovariancesEx")
  BIND(set_corner_undistortion, "amdAprilTagsSetCornerUndistortion")
  BIND(get_undistorted_detections, "amdAprilTagsGetUndistortedDetections")
  BIND(set_raw_shift, "amdAprilTagsSetRawShift")
  BIND(set_tag_table, "amdAprilTagsSetTagTable")
#undef BIND
  return a;
}

// Family strings the reference accepts as parameter values (src/apriltag_node.cpp:47-58).
const char* const kKnownFamilyStrings[] = {"tag36h11", "tag16h5", "tag25h9", "tag36h10", "circle21h7",
                                           "circle49h12", "custom48h12", "standard41h12", "standard52h13"};

// Encodings the node's input conversion accepts (src/apriltag_node.cpp:76-82).
// NodeOptions::quad_sigma on a freshly created handle (an identity value changes nothing: no plane, no launch)
void apply_quad_sigma(amdAprilTagsHandle detector, double quad_sigma) {
  const int error = api().set_quad_sigma(detector, static_cast<float>(quad_sigma));
  if (error != 0)
    throw std::runtime_error("'quad_sigma' " + std::to_string(quad_sigma) + " refused (error code " + std::to_string(error) + ")");
}

amdAprilTagsCameraModel_t to_abi(const CameraModel& m) {
  amdAprilTagsCameraModel_t o;
  for (int i = 0; i < 9; i++) { o.K[i] = m.k[i]; o.Knew[i] = m.knew[i]; }
  for (int i = 0; i < 5; i++) o.D[i] = m.d[i];
  return o;
}

amdAprilTagsCameraModelEx_t to_abi(const CameraModelEx& m) {
  amdAprilTagsCameraModelEx_t o = {};
  o.kind = m.kind;
  for (int i = 0; i < 9; i++) { o.K[i] = m.k[i]; o.R[i] = m.r[i]; o.Knew[i] = m.knew[i]; }
  for (int i = 0; i < 8; i++) o.D[i] = m.d[i];
  return o;
}

bool rectifying(const NodeOptions& opt) { return opt.rectify || opt.rectify_full; }
bool undistorting(const NodeOptions& opt) { return opt.undistort_corners; }

// The model of a stream's CameraInfo under the options: RectificationModelEx with rectify_full, otherwise RectificationModel (plumb_bob
// alone, no rotation) in the same form.  Throws what they throw.
CameraModelEx stream_model(const NodeOptions& opt, const CameraInfo& info) {
  if (opt.rectify_full || opt.undistort_corners) return RectificationModelEx(info);
  const CameraModel m = RectificationModel(info);
  CameraModelEx e;
  e.k = m.k; e.knew = m.knew;
  for (int i = 0; i < 5; i++) e.d[i] = m.d[i];
  e.r = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  return e;
}

// n models to the handle: the Ex call with rectify_full, the plumb_bob call otherwise (as before there was another)
int apply_models(amdAprilTagsHandle detector, const NodeOptions& opt, const CameraModelEx* models, uint32_t n) {
  if (opt.rectify_full) {
    std::vector<amdAprilTagsCameraModelEx_t> abi(n);
    for (uint32_t i = 0; i < n; i++) abi[i] = to_abi(models[i]);
    return api().set_rectification_ex(detector, n, abi.data());
  }
  std::vector<amdAprilTagsCameraModel_t> abi(n);
  for (uint32_t i = 0; i < n; i++) {
    CameraModel m;
    m.k = models[i].k; m.knew = models[i].knew;
    for (int j = 0; j < 5; j++) m.d[j] = models[i].d[j];
    abi[i] = to_abi(m);
  }
  return api().set_rectification(detector, n, abi.data());
}

bool resizing(const NodeOptions& opt) { return opt.resize_width != 0 && opt.resize_height != 0; }

// NodeOptions::undistort_corners: the stream's model as the library must see it -- the camera of the DETECTED image, so with
// NodeOptions::resize_width x resize_height K and Knew scaled as pose_camera scales the pose's camera.
CameraModelEx detected_model(const NodeOptions& opt, const CameraInfo& info) {
  CameraModelEx m = stream_model(opt, info);
  if (resizing(opt) && info.width != 0 && info.height != 0) {
    for (int c = 0; c < 3; c++) {
      m.k[c] = m.k[c] * static_cast<double>(opt.resize_width) / static_cast<double>(info.width);
      m.k[3 + c] = m.k[3 + c] * static_cast<double>(opt.resize_height) / static_cast<double>(info.height);
      m.knew[c] = m.knew[c] * static_cast<double>(opt.resize_width) / static_cast<double>(info.width);
      m.knew[3 + c] = m.knew[3 + c] * static_cast<double>(opt.resize_height) / static_cast<double>(info.height);
    }
  }
  return m;
}

// n such models to the handle
int apply_corner_models(amdAprilTagsHandle detector, const CameraModelEx* models, uint32_t n) {
  std::vector<amdAprilTagsCameraModelEx_t> abi(n);
  for (uint32_t i = 0; i < n; i++) abi[i] = to_abi(models[i]);
  return api().set_corner_undistortion(detector, n, abi.data());
}

void check_camera_options(const NodeOptions& opt) {
  if (undistorting(opt) && rectifying(opt)) throw std::runtime_error("'undistort_corners' and 'rectify' exclude each other: a frame is resampled or read raw");
}

// The camera matrix the pose is computed with: Knew of the stream's model with NodeOptions::rectify, K otherwise -- and with
// NodeOptions::resize_width x resize_height that camera scaled to the resized image (image_proc's convention: the first row times
// resize_width / width, the second times resize_height / height).
std::array<double, 9> pose_camera(const NodeOptions& opt, const CameraInfo& info) {
  std::array<double, 9> k = rectifying(opt) || undistorting(opt) ? stream_model(opt, info).knew : info.k;
  if (resizing(opt) && info.width != 0 && info.height != 0) {
    for (int c = 0; c < 3; c++) {
      k[c] = k[c] * static_cast<double>(opt.resize_width) / static_cast<double>(info.width);
      k[3 + c] = k[3 + c] * static_cast<double>(opt.resize_height) / static_cast<double>(info.height);
    }
  }
  return k;
}

void apply_resize(amdAprilTagsHandle detector, const NodeOptions& opt) {
  if (!resizing(opt)) return;
  const amdAprilTagsSize_t size = {opt.resize_width, opt.resize_height};
  const int error = api().set_resize(detector, 1, &size);
  if (error != 0)
    throw std::runtime_error("'resize_width' x 'resize_height' " + std::to_string(opt.resize_width) + " x " +
                             std::to_string(opt.resize_height) + " refused (error code " + std::to_string(error) + ")");
}

// NodeOptions::bundles on a freshly created handle (the node has one family: family_index 0)
void apply_bundles(amdAprilTagsHandle detector, const NodeOptions& opt) {
  if (opt.bundles.empty()) return;
  std::vector<std::vector<amdAprilTagsBundleMember_t>> members(opt.bundles.size());
  std::vector<amdAprilTagsBundle_t> abi(opt.bundles.size());
  for (size_t b = 0; b < opt.bundles.size(); b++) {
    const Bundle& in = opt.bundles[b];
    if (in.name.size() > 31) throw std::runtime_error("'bundles': the name '" + in.name + "' has more than 31 characters");
    for (const BundleMember& m : in.members) members[b].push_back({0u, m.id, m.x, m.y, m.size});
    abi[b] = {};
    abi[b].members = members[b].data();
    abi[b].nmembers = static_cast<uint32_t>(members[b].size());
    abi[b].max_hamming = in.max_hamming;
    abi[b].min_decision_margin = static_cast<float>(in.min_decision_margin);
    abi[b].min_tags = in.min_tags;
    std::strncpy(abi[b].name, in.name.c_str(), sizeof(abi[b].name) - 1);
  }
  const int error = api().set_bundles(detector, static_cast<uint32_t>(abi.size()), abi.data());
  if (error != 0) throw std::runtime_error("'bundles' refused (error code " + std::to_string(error) + ")");
}

// NodeOptions::rigid_bundles on a freshly created handle (family_index 0): the member's quaternion, divided by its norm, as a rotation
void apply_rigid_bundles(amdAprilTagsHandle detector, const NodeOptions& opt) {
  if (opt.rigid_bundles.empty()) return;
  if (!opt.bundles.empty()) throw std::runtime_error("'bundles' and 'rigid_bundles' are both set: one kind of bundle is on at a time");
  std::vector<std::vector<amdAprilTagsBundleMemberEx_t>> members(opt.rigid_bundles.size());
  std::vector<amdAprilTagsBundleEx_t> abi(opt.rigid_bundles.size());
  for (size_t b = 0; b < opt.rigid_bundles.size(); b++) {
    const RigidBundle& in = opt.rigid_bundles[b];
    if (in.name.size() > 31) throw std::runtime_error("'rigid_bundles': the name '" + in.name + "' has more than 31 characters");
    for (const RigidBundleMember& m : in.members) {
      const double n = std::sqrt(m.qw * m.qw + m.qx * m.qx + m.qy * m.qy + m.qz * m.qz);
      if (!(n > 0.0)) throw std::runtime_error("'rigid_bundles': tag " + std::to_string(m.id) + " of '" + in.name + "' has a zero quaternion");
      const double w = m.qw / n, x = m.qx / n, y = m.qy / n, z = m.qz / n;
      amdAprilTagsBundleMemberEx_t o = {};
      o.family_index = 0u; o.id = m.id; o.size = m.size;
      o.R[0] = 1 - 2 * (y * y + z * z); o.R[1] = 2 * (x * y - z * w);     o.R[2] = 2 * (x * z + y * w);
      o.R[3] = 2 * (x * y + z * w);     o.R[4] = 1 - 2 * (x * x + z * z); o.R[5] = 2 * (y * z - x * w);
      o.R[6] = 2 * (x * z - y * w);     o.R[7] = 2 * (y * z + x * w);     o.R[8] = 1 - 2 * (x * x + y * y);
      o.t[0] = m.x; o.t[1] = m.y; o.t[2] = m.z;
      members[b].push_back(o);
    }
    abi[b] = {};
    abi[b].members = members[b].data();
    abi[b].nmembers = static_cast<uint32_t>(members[b].size());
    abi[b].max_hamming = in.max_hamming;
    abi[b].min_decision_margin = static_cast<float>(in.min_decision_margin);
    abi[b].min_tags = in.min_tags;
    abi[b].iterations = in.iterations;
    std::strncpy(abi[b].name, in.name.c_str(), sizeof(abi[b].name) - 1);
  }
  const int error = api().set_bundles_ex(detector, static_cast<uint32_t>(abi.size()), abi.data());
  if (error != 0) throw std::runtime_error("'rigid_bundles' refused (error code " + std::to_string(error) + ")");
}

// NodeOptions::tags at construction: what can be refused without a handle
void check_tags(const NodeOptions& opt) {
  if (opt.tags.size() > AMDAT_MAX_TAG_ENTRIES) throw std::runtime_error("'tags': at most " + std::to_string(AMDAT_MAX_TAG_ENTRIES) + " entries");
  std::set<uint32_t> ids;
  for (const TagSpec& t : opt.tags) {
    if (!t.family.empty() && t.family != opt.tag_family)
      throw std::runtime_error("'tags': family '" + t.family + "' is not the node's tag_family '" + opt.tag_family + "'");
    if (t.frame.size() > 47) throw std::runtime_error("'tags': frame '" + t.frame + "' is longer than 47 characters");
    if (!(t.size >= 0.0) || !std::isfinite(t.size)) throw std::runtime_error("'tags': the size of id " + std::to_string(t.id) + " is negative or not finite");
    if (t.id >= AMDAT_TAG_ID_ANY) throw std::runtime_error("'tags': id " + std::to_string(t.id) + " is no tag id");
    if (!ids.insert(t.id).second) throw std::runtime_error("'tags': id " + std::to_string(t.id) + " is listed twice");
  }
  if (opt.tags_listed_only && opt.tags.empty()) throw std::runtime_error("'tags_listed_only' needs 'tags'");
}

// NodeOptions::tags on a freshly created handle (one family: index 0)
void apply_tag_table(amdAprilTagsHandle detector, const NodeOptions& opt) {
  if (opt.tags.empty()) return;
  std::vector<amdAprilTagsTagEntry_t> abi(opt.tags.size());
  for (size_t i = 0; i < abi.size(); i++) abi[i] = {0u, opt.tags[i].id, static_cast<float>(opt.tags[i].size), 0u};
  const int error = api().set_tag_table(detector, static_cast<uint32_t>(abi.size()), abi.data(), opt.tags_listed_only ? 1u : 0u);
  if (error != 0) throw std::runtime_error("'tags' refused (error code " + std::to_string(error) + ")");
}

// The TF child frame of tag `id`: its NodeOptions::tags frame where it has one, "family:id" otherwise
std::string tag_child_frame(const NodeOptions& opt, uint32_t id) {
  for (const TagSpec& t : opt.tags)
    if (t.id == id && !t.frame.empty()) return t.frame;
  return opt.tag_family + ":" + std::to_string(id);
}

// NodeOptions::pose_refinement on a freshly created handle
void apply_pose_refinement(amdAprilTagsHandle detector, const NodeOptions& opt) {
  if (opt.pose_refinement == 0) return;
  const int error = api().set_pose_refinement(detector, opt.pose_refinement);
  if (error != 0) throw std::runtime_error("'pose_refinement' " + std::to_string(opt.pose_refinement) + " refused (error code " + std::to_string(error) + ")");
}

// NodeOptions::pose_covariance_sigma_px on a freshly created handle
void apply_pose_covariance(amdAprilTagsHandle detector, const NodeOptions& opt) {
  if (opt.pose_covariance_sigma_px == 0.0) return;
  const int error = api().set_pose_covariance(detector, opt.pose_covariance_sigma_px);
  if (error != 0)
    throw std::runtime_error("'pose_covariance_sigma_px' " + std::to_string(opt.pose_covariance_sigma_px) + " refused (error code " + std::to_string(error) + ")");
}

// NodeOptions::pose_refinement: the pose of every tag of frame `frame` of the submission that just returned becomes the chosen refined
// one (amdAprilTagsGetRefinedPoses: record i belongs to tag i) -- translation and column-major orientation in float, as the library
// forms them from the homography pose.  (The node runs the default corner convention: R as solved.)
// NodeOptions::pose_covariance_sigma_px with it: covs[i] is the chosen pose's covariance, the 36 doubles as the library hands them
// out (row-major in ROS' order), or zeros where the record's is not valid; off, covs stays empty.
// invalid: the marks of undistort_tags (NodeOptions::undistort_corners).  A tag marked there keeps the pose that call gave it: its refined
// record is AMDAT_POSE_DEGENERATE with zero fields, which is no pose (and its covariance record is not valid: zeros).
bool refine_tags(amdAprilTagsHandle detector, const NodeOptions& opt, uint32_t frame, amdAprilTagsID_t* tags, uint32_t num_detections,
                 std::vector<std::array<double, 36>>* covs, const std::vector<uint8_t>& invalid) {
  covs->clear();
  if (opt.pose_refinement == 0) return true;
  if (opt.pose_covariance_sigma_px != 0.0) {
    std::vector<amdAprilTagsPoseCovariance_t> crecs(num_detections ? num_detections : 1u);
    uint32_t cn = 0;
    if (api().get_refined_pose_covariances(detector, frame, crecs.data(), num_detections, &cn) != 0 || cn != num_detections) return false;
    covs->resize(num_detections);
    for (uint32_t i = 0; i < cn; i++)
      for (int k = 0; k < 36; k++) (*covs)[i][k] = (crecs[i].valid & 1u) ? crecs[i].cov[k] : 0.0;
  }
  std::vector<amdAprilTagsRefinedPose_t> recs(num_detections ? num_detections : 1u);
  uint32_t n = 0;
  if (api().get_refined_poses(detector, frame, recs.data(), num_detections, &n) != 0 || n != num_detections) return false;
  for (uint32_t i = 0; i < n; i++) {
    if (i < invalid.size() && invalid[i]) continue;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) tags[i].orientation[c * 3 + r] = static_cast<float>(recs[i].R[r * 3 + c]);
    for (int k = 0; k < 3; k++) tags[i].translation[k] = static_cast<float>(recs[i].t[k]);
  }
  return true;
}

// NodeOptions::undistort_corners: the pose of every tag of frame `frame` of the submission that just returned becomes its undistorted
// twin's (amdAprilTagsGetUndistortedDetections: record i belongs to tag i), formed in float as the library forms a tag's from the
// record's; an invalid twin gives a zero translation and the identity, and is marked in `invalid` (one entry per tag; empty with the
// mode off).  Corners and centre stay the raw frame's.
bool undistort_tags(amdAprilTagsHandle detector, const NodeOptions& opt, uint32_t frame, amdAprilTagsID_t* tags, uint32_t num_detections,
                    std::vector<uint8_t>* invalid) {
  invalid->clear();
  if (!undistorting(opt)) return true;
  std::vector<amdAprilTagsUndistortedDetection_t> recs(num_detections ? num_detections : 1u);
  uint32_t n = 0;
  if (api().get_undistorted_detections(detector, frame, recs.data(), num_detections, &n) != 0 || n != num_detections) return false;
  for (uint32_t i = 0; i < n; i++) {
    const bool ok = recs[i].status == AMDAT_UNDISTORT_OK;
    invalid->push_back(ok ? 0 : 1);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) tags[i].orientation[c * 3 + r] = ok ? static_cast<float>(recs[i].R[r * 3 + c]) : (r == c ? 1.0f : 0.0f);
    for (int k = 0; k < 3; k++) tags[i].translation[k] = ok ? static_cast<float>(recs[i].t[k]) : 0.0f;
  }
  return true;
}

Quaternion quaternion_from_colmajor(const float* o);

// The bundle records of the first nframes frames of the submission that just returned (frame-major), and per frame one transform for
// every solved bundle appended to tfs[f]: child frame "bundle:<name>", the frame's camera info header, as for tags.
bool collect_bundles(amdAprilTagsHandle detector, const NodeOptions& opt, uint32_t nframes, const Header* const* headers,
                     std::vector<std::vector<BundlePose>>* poses, std::vector<TransformStamped>* const* tfs) {
  const size_t nb = opt.bundles.size();
  poses->assign(nframes, std::vector<BundlePose>());
  if (nb == 0) return true;
  std::vector<amdAprilTagsBundlePose_t> recs(static_cast<size_t>(nframes) * nb);
  if (api().get_bundle_poses(detector, recs.data(), nframes) != 0) return false;
  for (uint32_t f = 0; f < nframes; f++) {
    for (size_t b = 0; b < nb; b++) {
      const amdAprilTagsBundlePose_t& r = recs[f * nb + b];
      BundlePose p;
      p.name = opt.bundles[b].name;
      p.status = r.status; p.ntags = r.ntags; p.nskipped = r.nskipped; p.sq_err_sum = r.sq_err_sum;
      for (int i = 0; i < 9; i++) p.R[i] = r.R[i];
      for (int i = 0; i < 3; i++) p.t[i] = r.t[i];
      (*poses)[f].push_back(p);
      if (r.status != AMDAT_BUNDLE_SOLVED) continue;
      TransformStamped tf;
      tf.header = *headers[f];
      tf.child_frame_id = "bundle:" + p.name;
      tf.transform.translation.x = r.t[0];
      tf.transform.translation.y = r.t[1];
      tf.transform.translation.z = r.t[2];
      float o[9];   // column-major float, the form a tag's orientation has
      for (int rr = 0; rr < 3; rr++)
        for (int c = 0; c < 3; c++) o[c * 3 + rr] = static_cast<float>(r.R[rr * 3 + c]);
      tf.transform.rotation = quaternion_from_colmajor(o);
      tfs[f]->push_back(tf);
    }
  }
  return true;
}

// The same for NodeOptions::rigid_bundles: the records of amdAprilTagsGetBundlePosesEx, and one transform per solved bundle from the
// chosen pose.
bool collect_rigid_bundles(amdAprilTagsHandle detector, const NodeOptions& opt, uint32_t nframes, const Header* const* headers,
                           std::vector<std::vector<RigidBundlePose>>* poses, std::vector<TransformStamped>* const* tfs) {
  const size_t nb = opt.rigid_bundles.size();
  poses->assign(nframes, std::vector<RigidBundlePose>());
  if (nb == 0) return true;
  std::vector<amdAprilTagsBundlePoseEx_t> recs(static_cast<size_t>(nframes) * nb);
  if (api().get_bundle_poses_ex(detector, recs.data(), nframes) != 0) return false;
  // NodeOptions::pose_covariance_sigma_px: the chosen pose's covariance beside every record, zeros where it is not valid
  std::vector<amdAprilTagsPoseCovariance_t> crecs;
  if (opt.pose_covariance_sigma_px != 0.0) {
    crecs.resize(recs.size());
    if (api().get_bundle_pose_covariances_ex(detector, crecs.data(), nframes) != 0) return false;
  }
  for (uint32_t f = 0; f < nframes; f++) {
    for (size_t b = 0; b < nb; b++) {
      const amdAprilTagsBundlePoseEx_t& r = recs[f * nb + b];
      RigidBundlePose p;
      p.name = opt.rigid_bundles[b].name;
      p.status = r.status; p.ntags = r.ntags; p.nskipped = r.nskipped; p.seed = r.seed; p.chosen = r.chosen;
      p.err = r.err; p.sq_err_sum = r.sq_err_sum; p.err_alt = r.err_alt; p.sq_err_sum_alt = r.sq_err_sum_alt;
      for (int i = 0; i < 9; i++) { p.R[i] = r.R[i]; p.R_alt[i] = r.R_alt[i]; }
      for (int i = 0; i < 3; i++) { p.t[i] = r.t[i]; p.t_alt[i] = r.t_alt[i]; }
      if (!crecs.empty() && (crecs[f * nb + b].valid & 1u))
        for (int i = 0; i < 36; i++) p.covariance[i] = crecs[f * nb + b].cov[i];
      (*poses)[f].push_back(p);
      if (r.status != AMDAT_BUNDLE_SOLVED) continue;
      TransformStamped tf;
      tf.header = *headers[f];
      tf.child_frame_id = "bundle:" + p.name;
      tf.transform.translation.x = r.t[0];
      tf.transform.translation.y = r.t[1];
      tf.transform.translation.z = r.t[2];
      float o[9];   // column-major float, the form a tag's orientation has
      for (int rr = 0; rr < 3; rr++)
        for (int c = 0; c < 3; c++) o[c * 3 + rr] = static_cast<float>(r.R[rr * 3 + c]);
      tf.transform.rotation = quaternion_from_colmajor(o);
      tfs[f]->push_back(tf);
    }
  }
  return true;
}

// NodeOptions::rig_cameras on a freshly created handle of S streams: one extrinsic per stream, beside rigid_bundles.
void apply_rig(amdAprilTagsHandle detector, const NodeOptions& opt, uint32_t S) {
  if (opt.rig_cameras.empty()) return;
  if (opt.rig_cameras.size() != S) throw std::runtime_error("'rig_cameras' must give one camera per stream");
  if (opt.rigid_bundles.empty()) throw std::runtime_error("'rig_cameras' is set without 'rigid_bundles': the rig solves rigid bundles");
  std::vector<amdAprilTagsRigCamera_t> cams(S);
  for (uint32_t s = 0; s < S; s++) {
    for (int i = 0; i < 9; i++) cams[s].R[i] = opt.rig_cameras[s].R[i];
    for (int i = 0; i < 3; i++) cams[s].t[i] = opt.rig_cameras[s].t[i];
  }
  const int error = api().set_rig(detector, S, cams.data());
  if (error != 0) throw std::runtime_error("'rig_cameras' refused (error code " + std::to_string(error) + ")");
}

// NodeOptions::rig_cameras: the records of amdAprilTagsGetRigBundlePoses for group 0, the round, and one transform per solved bundle
// from the chosen pose under the rig frame.  who[i]: the stream of batch slot i.
bool collect_rig_bundles(amdAprilTagsHandle detector, const NodeOptions& opt, const std::vector<uint32_t>& who, const Header& first,
                         std::vector<RigBundlePose>* poses, std::vector<TransformStamped>* tfs) {
  poses->clear();
  const size_t nb = opt.rigid_bundles.size();
  if (opt.rig_cameras.empty() || nb == 0) return true;
  std::vector<amdAprilTagsRigBundlePose_t> recs(nb);
  if (api().get_rig_bundle_poses(detector, recs.data(), 1) != 0) return false;
  for (size_t b = 0; b < nb; b++) {
    const amdAprilTagsRigBundlePose_t& r = recs[b];
    RigBundlePose p;
    p.name = opt.rigid_bundles[b].name;
    p.status = r.status; p.nobs = r.nobs; p.nskipped = r.nskipped; p.ndropped = r.ndropped; p.ncams = r.ncams;
    p.seed_stream = r.seed_frame < who.size() ? who[r.seed_frame] : 0; p.seed = r.seed; p.chosen = r.chosen;
    p.err = r.err; p.sq_err_sum = r.sq_err_sum; p.err_alt = r.err_alt; p.sq_err_sum_alt = r.sq_err_sum_alt;
    for (int i = 0; i < 9; i++) { p.R[i] = r.R[i]; p.R_alt[i] = r.R_alt[i]; }
    for (int i = 0; i < 3; i++) { p.t[i] = r.t[i]; p.t_alt[i] = r.t_alt[i]; }
    poses->push_back(p);
    if (r.status != AMDAT_BUNDLE_SOLVED) continue;
    TransformStamped tf;
    tf.header = first;
    tf.header.frame_id = opt.rig_frame_id;
    tf.child_frame_id = "rig_bundle:" + p.name;
    tf.transform.translation.x = r.t[0];
    tf.transform.translation.y = r.t[1];
    tf.transform.translation.z = r.t[2];
    float o[9];   // column-major float, the form a tag's orientation has
    for (int rr = 0; rr < 3; rr++)
      for (int c = 0; c < 3; c++) o[c * 3 + rr] = static_cast<float>(r.R[rr * 3 + c]);
    tf.transform.rotation = quaternion_from_colmajor(o);
    tfs->push_back(tf);
  }
  return true;
}

int bytes_per_pixel(const std::string& enc) {
  if (enc == "mono8") return 1;
  if (enc == "rgb8" || enc == "bgr8") return 3;
  if (enc == "rgba8" || enc == "bgra8") return 4;
  return 0;
}
// The raw formats the single-stream node hands through beside the five above: bytes per sample, 0 for any
// other string.  (The multi-stream shell converts into its batch slots itself and keeps to the five.)
int raw_bytes_per_sample(const std::string& enc) {
  static const char* const k8[] = {"bayer_rggb8", "bayer_bggr8", "bayer_gbrg8", "bayer_grbg8"};
  static const char* const k16[] = {"mono16", "bayer_rggb16", "bayer_bggr16", "bayer_gbrg16", "bayer_grbg16"};
  for (const char* n : k8) if (enc == n) return 1;
  for (const char* n : k16) if (enc == n) return 2;
  return 0;
}

// `backends` is the reference's VPI backend flag string: one name or a comma-separated list
// (test/isaac_ros_apriltag_backends_compare_test.py:33-37 uses 'CPU', 'CUDA', 'PVA').  Names the reference's
// VPI builds know plus this library's own.  Throws on an unknown name.
std::set<std::string> parse_backends(const std::string& backends) {
  static const char* const kKnown[] = {"CPU", "CUDA", "PVA", "VIC", "NVENC", "OFA", "ALL", "HIP", "GPU"};
  std::set<std::string> out;
  size_t pos = 0;
  while (pos <= backends.size()) {
    size_t comma = backends.find(',', pos);
    if (comma == std::string::npos) comma = backends.size();
    std::string tok = backends.substr(pos, comma - pos);
    const size_t a = tok.find_first_not_of(" \t"), b = tok.find_last_not_of(" \t");
    tok = (a == std::string::npos) ? std::string() : tok.substr(a, b - a + 1);
    for (auto& ch : tok) ch = static_cast<char>(std::toupper(static_cast<unsigned char>(ch)));
    bool known = false;
    for (const char* k : kKnown) known |= tok == k;
    if (!known) throw std::runtime_error("Unrecognized backend '" + tok + "' in 'backends' parameter");
    out.insert(tok);
    pos = comma + 1;
  }
  return out;
}

// Rotation matrix (column-major 3x3 float, as cuAprilTagsID_t::orientation) -> quaternion, the
// construction Eigen::Quaternion<float>(matrix) performs in ToTransformMsg (src/apriltag_node.cpp:409-427).
Quaternion quaternion_from_colmajor(const float* o) {
  auto m = [&](int r, int c) { return o[c * 3 + r]; };
  float q[4];  // x y z w
  float t = m(0, 0) + m(1, 1) + m(2, 2);
  if (t > 0.0f) {
    t = std::sqrt(t + 1.0f);
    q[3] = 0.5f * t;
    t = 0.5f / t;
    q[0] = (m(2, 1) - m(1, 2)) * t;
    q[1] = (m(0, 2) - m(2, 0)) * t;
    q[2] = (m(1, 0) - m(0, 1)) * t;
  } else {
    int i = 0;
    if (m(1, 1) > m(0, 0)) i = 1;
    if (m(2, 2) > m(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(m(i, i) - m(j, j) - m(k, k) + 1.0f);
    q[i] = 0.5f * t;
    t = 0.5f / t;
    q[3] = (m(k, j) - m(j, k)) * t;
    q[j] = (m(j, i) + m(i, j)) * t;
    q[k] = (m(k, i) + m(i, k)) * t;
  }
  Quaternion out;
  out.x = q[0]; out.y = q[1]; out.z = q[2]; out.w = q[3];
  return out;
}

// AprilTagDetectionArray + TF transforms of one frame from the detector's records (src/apriltag_node.cpp:499-549)
void assemble_messages(const amdAprilTagsID_t* tags, uint32_t num_detections, const Header& info_header, const NodeOptions& opt,
                       AprilTagDetectionArray* msg_out, std::vector<TransformStamped>* tfs_out,
                       const std::vector<std::array<double, 36>>* covs = nullptr) {
  AprilTagDetectionArray& msg = *msg_out;
  std::vector<TransformStamped>& tfs = *tfs_out;
  const std::string& family = opt.tag_family;
  msg.header = info_header;  // camera_info header, not the image header (src/apriltag_node.cpp:501)
  for (uint32_t i = 0; i < num_detections; i++) {
    const amdAprilTagsID_t& d = tags[i];
    AprilTagDetection det;
    det.family = family;
    det.id = d.id;
    for (int c = 0; c < 4; c++) {
      det.corners[c].x = d.corners[c].x;
      det.corners[c].y = d.corners[c].y;
    }
    // The reference intersects the diagonals in slope/intercept form, which divides by zero when a
    // diagonal is vertical (src/apriltag_node.cpp:519-530); the library reports H(0,0) directly.
    det.center.x = d.center.x;
    det.center.y = d.center.y;
    TransformStamped tf;
    tf.header = info_header;
    tf.child_frame_id = tag_child_frame(opt, d.id);   // (NodeOptions::tags: the tag's frame name; "family:id" without one)
    tf.transform.translation.x = d.translation[0];
    tf.transform.translation.y = d.translation[1];
    tf.transform.translation.z = d.translation[2];
    tf.transform.rotation = quaternion_from_colmajor(d.orientation);
    tfs.push_back(tf);
    det.pose.pose.pose.position.x = tf.transform.translation.x;
    det.pose.pose.pose.position.y = tf.transform.translation.y;
    det.pose.pose.pose.position.z = tf.transform.translation.z;
    det.pose.pose.pose.orientation = tf.transform.rotation;
    if (covs && i < covs->size()) det.pose.pose.covariance = (*covs)[i];   // (the doubles as they are: no conversion)
    msg.detections.push_back(det);
  }
}

// Backend / family validation of the constructor (src/apriltag_node.cpp:575-599): returns the family enum, throws with
// the reference's text otherwise.  cuapriltags_mode: exactly {CUDA} was asked for (tag36h11 only).
int validate_family(const NodeOptions& options, bool* cuapriltags_mode) {
  const std::set<std::string> backends = parse_backends(options.backends);
  *cuapriltags_mode = backends.size() == 1 && *backends.begin() == "CUDA";
  std::set<std::string> supported;
  if (*cuapriltags_mode) {
    supported.insert("tag36h11");
  } else {
    // any other backend list: the reference runs VPI, whose family table is src/apriltag_node.cpp:47-58;
    // here the families this library can decode = those with a code table (built in or registered by the host)
    for (const char* f : kKnownFamilyStrings)
      if (api().family_from_name(f) >= 0) supported.insert(f);
    if (api().family_from_name(options.tag_family.c_str()) >= 0) supported.insert(options.tag_family);
  }
  if (supported.find(options.tag_family) == supported.end()) {
    std::ostringstream os;
    os << "Tag family not supported by specified backend: '" << options.tag_family << "'" << std::endl;
    os << "'tag_family' parameter must be one of:" << std::endl;
    for (const auto& f : supported) os << f << std::endl;
    std::fprintf(stderr, "[apriltag_node] FATAL: Tag family not supported by specified backend: '%s'\n", options.tag_family.c_str());
    throw std::runtime_error(os.str());
  }
  return api().family_from_name(options.tag_family.c_str());
}

}  // namespace

CameraModel RectificationModel(const CameraInfo& info) {
  if (!info.distortion_model.empty() && info.distortion_model != "plumb_bob")
    throw std::runtime_error("'rectify' supports the distortion model 'plumb_bob' only, not '" + info.distortion_model + "'");
  if (info.d.size() > 5)
    throw std::runtime_error("'rectify': 'plumb_bob' has five coefficients (k1, k2, p1, p2, k3), camera_info carries " +
                             std::to_string(info.d.size()));
  CameraModel m;
  m.k = info.k;
  for (size_t i = 0; i < info.d.size(); i++) m.d[i] = info.d[i];
  if (info.p[0] != 0.0) {
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) m.knew[r * 3 + c] = info.p[r * 4 + c];
  } else {
    m.knew = info.k;
  }
  return m;
}

CameraModelEx RectificationModelEx(const CameraInfo& info) {
  static const char* const names[3] = {"plumb_bob", "rational_polynomial", "equidistant"};
  static const size_t ncoef[3] = {5, 8, 4};
  CameraModelEx m;
  const std::string& name = info.distortion_model;
  if (name.empty() || name == names[0]) m.kind = 0;
  else if (name == names[1]) m.kind = 1;
  else if (name == names[2]) m.kind = 2;
  else
    throw std::runtime_error("'rectify_full' supports the distortion models 'plumb_bob', 'rational_polynomial' and 'equidistant', not '" +
                             name + "'");
  if (info.d.size() > ncoef[m.kind])
    throw std::runtime_error(std::string("'rectify_full': '") + names[m.kind] + "' has " + std::to_string(ncoef[m.kind]) +
                             " coefficients, camera_info carries " + std::to_string(info.d.size()));
  m.k = info.k;
  for (size_t i = 0; i < info.d.size(); i++) m.d[i] = info.d[i];
  bool filled = false;
  for (double v : info.r) filled = filled || v != 0.0;
  if (filled) m.r = info.r;
  else m.r = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // a monocular driver leaves r at zero
  if (info.p[0] != 0.0) {
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) m.knew[r * 3 + c] = info.p[r * 4 + c];
  } else {
    m.knew = info.k;
  }
  return m;
}

struct AprilTagNode::Impl {
  NodeOptions opt;
  DetectionsCallback on_detections;
  TransformsCallback on_transforms;
  // lazily created on the first frame (src/apriltag_node.cpp:618-620)
  bool initialized = false;
  amdAprilTagsHandle detector = nullptr;
  int family_enum = -1;
  uint32_t width = 0, height = 0;
  void* d_input = nullptr;   // staging for host images
  size_t d_input_bytes = 0;
  amdAprilTagsStream stream = nullptr;   // the host-to-device copy and the detection are ordered on it: one host wait per frame

  // exactly {CUDA}: the reference runs cuAprilTags, which decodes tag36h11 only (src/apriltag_node.cpp:429-432)
  bool cuapriltags_mode = false;
  std::vector<BundlePose> last_bundles;   // NodeOptions::bundles: the records of the last published frame
  std::vector<RigidBundlePose> last_rigid;   // NodeOptions::rigid_bundles: the same

  void Initialize(const Image& image, const CameraInfo& info) {
    if (opt.max_tags <= 0) throw std::runtime_error("'max_tags' must be positive");
    check_camera_options(opt);
    if (detector) { api().destroy(detector); detector = nullptr; }   // left over from a failed attempt
    // intrinsics from K, double -> float as the reference does (src/apriltag_node.cpp:442-447)
    amdAprilTagsConfig_t cfg;
    const bool resize = resizing(opt);   // the handle has the size the frames are resized to
    api().default_config(&cfg, resize ? opt.resize_width : info.width, resize ? opt.resize_height : info.height);
    cfg.tile_size = opt.tile_size;
    cfg.decimate = opt.decimate;
    cfg.num_families = 1;
    cfg.families[0] = static_cast<amdAprilTagsFamily>(family_enum);
    const std::array<double, 9> k = pose_camera(opt, info);   // (rectify: Knew; throws on a model it cannot rectify; resize: scaled)
    cfg.intrinsics.fx = static_cast<float>(k[0]);
    cfg.intrinsics.fy = static_cast<float>(k[4]);
    cfg.intrinsics.cx = static_cast<float>(k[2]);
    cfg.intrinsics.cy = static_cast<float>(k[5]);
    // the VPI path also passes the skew K[1] (src/apriltag_node.cpp:215-225); cuAprilTags has no such field
    cfg.skew = cuapriltags_mode ? 0.0f : static_cast<float>(k[1]);
    cfg.tag_size = static_cast<float>(opt.size);
    cfg.max_batch = 1;
    const int error = api().create_ex(&detector, &cfg);
    if (error != 0) {
      // same text as src/apriltag_node.cpp:453-457 with the library name replaced
      throw std::runtime_error("Failed to create AprilTags detector (error code " + std::to_string(error) + ")");
    }
    apply_quad_sigma(detector, opt.quad_sigma);
    if (api().set_raw_shift(detector, opt.raw_shift) != 0)
      throw std::runtime_error("'raw_shift' " + std::to_string(opt.raw_shift) + " refused (0 .. 8)");
    if (rectifying(opt)) {
      const CameraModelEx model = stream_model(opt, info);
      const int rerr = apply_models(detector, opt, &model, 1);
      if (rerr != 0) throw std::runtime_error("'rectify': camera model refused (error code " + std::to_string(rerr) + ")");
    }
    if (undistorting(opt)) {
      const CameraModelEx model = detected_model(opt, info);
      const int rerr = apply_corner_models(detector, &model, 1);
      if (rerr != 0) throw std::runtime_error("'undistort_corners': camera model refused (error code " + std::to_string(rerr) + ")");
    }
    apply_resize(detector, opt);
    apply_bundles(detector, opt);
    apply_rigid_bundles(detector, opt);
    apply_tag_table(detector, opt);
    apply_pose_refinement(detector, opt);
    apply_pose_covariance(detector, opt);
    width = info.width;
    height = info.height;
    if (!stream && api().stream_create(&stream) != 0) throw std::runtime_error("stream creation failed");
    initialized = true;   // only now: a failed creation is retried (and reported) on the next frame
    (void)image;
  }

  void OnCameraFrame(const Image& image, const CameraInfo& info) {
    int bpp = bytes_per_pixel(image.encoding);
    if (cuapriltags_mode && opt.strict_cuapriltags_encodings && image.encoding != "rgb8" && image.encoding != "bgr8") {
      // the reference's cuAprilTags branch, text and all (src/apriltag_node.cpp:469-476)
      std::fprintf(stderr, "[apriltag_node] Unsupported image encoding: %s (only 'rgb8' or 'bgr8' supported)\n", image.encoding.c_str());
      throw std::runtime_error("cuAprilTags detector only supports 'rgb8' or 'bgr8' image input");
    }
    if (bpp == 0) {   // a Bayer or 16-bit frame goes to the detector as it arrived, as a colour frame does: the submission converts it
      bpp = raw_bytes_per_sample(image.encoding);
      if (bpp == 2 && image.is_bigendian) {   // (the library reads little-endian samples; big-endian ones are out of scope)
        std::fprintf(stderr, "[apriltag_node] Unsupported image encoding: %s with big-endian samples: frame dropped\n", image.encoding.c_str());
        return;
      }
    }
    if (bpp == 0) {
      // (a superset of the reference's cuAprilTags branch, which takes rgb8 / bgr8 only: NodeOptions::strict_cuapriltags_encodings)
      std::fprintf(stderr, "[apriltag_node] Unsupported image encoding: %s (supported: 'mono8', 'rgb8', 'bgr8', 'rgba8', 'bgra8'%s)\n",
                   image.encoding.c_str(), cuapriltags_mode ? "; the reference's cuAprilTags mode takes 'rgb8' / 'bgr8' only" : "");
      throw std::runtime_error("AprilTags detector only supports 'mono8', 'rgb8', 'bgr8', 'rgba8' or 'bgra8' image input");
    }
    // the detector and the conversion buffer are sized from camera_info at initialisation
    // (src/apriltag_node.cpp:228-231,257-260): a frame of another size is dropped before anything is written
    // (NodeOptions::resize_width x resize_height: a frame of any size the library resizes is taken)
    const bool size_ok = resizing(opt) ? image.width >= 1 && image.width <= 16384 && image.height >= 1 && image.height <= 16384 &&
                                             info.width == image.width && info.height == image.height
                                       : image.width == width && image.height == height && info.width == width && info.height == height;
    if (!size_ok ||
        static_cast<size_t>(image.step) < static_cast<size_t>(image.width) * bpp || image.data == nullptr) {
      std::fprintf(stderr, "[apriltag_node] image %ux%u (step %u) does not match the initialised size %ux%u: frame dropped\n",
                   image.width, image.height, image.step, width, height);
      return;
    }
    const uint8_t* dev_src = image.data;
    if (!image.is_device) {
      const size_t bytes = static_cast<size_t>(image.step) * image.height;
      if (bytes > d_input_bytes) {
        if (d_input) api().dev_free(d_input);
        d_input = nullptr;
        if (api().dev_alloc(&d_input, bytes) != 0) throw std::runtime_error("device allocation failed");
        d_input_bytes = bytes;
      }
      // enqueue-only, on the stream the detection runs on (image.data stays valid until the detection below has returned)
      if (api().copy_to_device_async(d_input, image.data, bytes, stream) != 0) {
        std::fprintf(stderr, "[apriltag_node] host-to-device copy failed\n");
        return;
      }
      dev_src = static_cast<const uint8_t*>(d_input);
    }
    // The frame goes to the detector in the encoding it arrived in -- the reference hands cuAprilTags its rgb8 / bgr8 uchar3 image
    // (src/apriltag_node.cpp:469-486), its VPI branch converts first (:275-282): here the threshold pass of the one call reads the
    // interleaved frame itself, there is no conversion launch (and no second device buffer) in between.
    amdAprilTagsImageInput_t input;
    input.width = image.width;
    input.height = image.height;
    input.dev_ptr = dev_src;
    input.pitch = image.step;
    uint32_t num_detections = 0;
    std::vector<amdAprilTagsID_t> tags(static_cast<size_t>(opt.max_tags));
    const int enc = api().encoding_from_name(image.encoding.c_str());
    // (the single-frame call keeps to the reference's five encodings: a raw frame is a batch of one)
    const int error = raw_bytes_per_sample(image.encoding)
                          ? api().detect_batch_color(detector, 1, &input, static_cast<amdAprilTagsEncoding>(enc), nullptr, tags.data(),
                                                     &num_detections, static_cast<uint32_t>(opt.max_tags), stream)
                          : api().detect_color(detector, &input, static_cast<amdAprilTagsEncoding>(enc), tags.data(), &num_detections,
                                               static_cast<uint32_t>(opt.max_tags), stream);
    if (error != 0) {
      // the reference logs and drops the frame (src/apriltag_node.cpp:494-497)
      std::fprintf(stderr, "[apriltag_node] Failed to run AprilTags detector (error code %d)\n", error);
      return;
    }
    std::vector<uint8_t> invalid;
    if (!undistort_tags(detector, opt, 0, tags.data(), num_detections, &invalid)) {
      std::fprintf(stderr, "[apriltag_node] undistorted detections not available: frame dropped\n");
      return;
    }
    std::vector<std::array<double, 36>> covs;
    if (!refine_tags(detector, opt, 0, tags.data(), num_detections, &covs, invalid)) {
      std::fprintf(stderr, "[apriltag_node] refined poses or their covariances not available: frame dropped\n");
      return;
    }
    AprilTagDetectionArray msg;
    std::vector<TransformStamped> tfs;
    assemble_messages(tags.data(), num_detections, info.header, opt, &msg, &tfs, &covs);
    {
      std::vector<std::vector<BundlePose>> poses;
      const Header* hdr = &info.header;
      std::vector<TransformStamped>* out = &tfs;
      if (!collect_bundles(detector, opt, 1, &hdr, &poses, &out)) {
        std::fprintf(stderr, "[apriltag_node] bundle records not available: frame dropped\n");
        return;
      }
      last_bundles = poses[0];
      std::vector<std::vector<RigidBundlePose>> rigid;
      if (!collect_rigid_bundles(detector, opt, 1, &hdr, &rigid, &out)) {
        std::fprintf(stderr, "[apriltag_node] rigid bundle records not available: frame dropped\n");
        return;
      }
      last_rigid = rigid[0];
    }
    if (on_detections) on_detections(msg);
    if (on_transforms) on_transforms(tfs);
  }
};

AprilTagNode::AprilTagNode(const NodeOptions& options) : impl_(new Impl()) {
  impl_->opt = options;
  // Backend selection (src/apriltag_node.cpp:575-582): this build has exactly one implementation, the
  // HIP detector; CPU / PVA backends of VPI do not exist here and support no family.
  // cuAprilTags when exactly CUDA was asked for, VPI otherwise; the HIP detector stands behind both, whatever
  // names the list holds (there is one implementation and no CPU fallback).
  impl_->family_enum = validate_family(options, &impl_->cuapriltags_mode);
  check_tags(options);
}

AprilTagNode::~AprilTagNode() {
  if (impl_) {
    if (impl_->detector) api().destroy(impl_->detector);
    if (impl_->stream) api().stream_destroy(impl_->stream);
    if (impl_->d_input) api().dev_free(impl_->d_input);
  }
}

void AprilTagNode::set_detections_callback(DetectionsCallback cb) { impl_->on_detections = std::move(cb); }
void AprilTagNode::set_transforms_callback(TransformsCallback cb) { impl_->on_transforms = std::move(cb); }
const NodeOptions& AprilTagNode::options() const { return impl_->opt; }
bool AprilTagNode::initialized() const { return impl_->initialized; }
const std::vector<BundlePose>& AprilTagNode::last_bundle_poses() const { return impl_->last_bundles; }
const std::vector<RigidBundlePose>& AprilTagNode::last_rigid_bundle_poses() const { return impl_->last_rigid; }

bool AprilTagNode::CameraImageCallback(const Image& image, const CameraInfo& camera_info) {
  if (image.header.stamp.sec != camera_info.header.stamp.sec || image.header.stamp.nanosec != camera_info.header.stamp.nanosec)
    return false;  // ExactTime synchroniser would not fire
  if (!impl_->initialized) impl_->Initialize(image, camera_info);
  impl_->OnCameraFrame(image, camera_info);
  return true;
}

// ---- AprilTagMultiCameraNode: S streams, one submission per round -----------------------------------------------------
struct AprilTagMultiCameraNode::Impl {
  NodeOptions opt;
  uint32_t S = 0;
  DetectionsCallback on_detections;
  TransformsCallback on_transforms;
  bool cuapriltags_mode = false, auto_flush = true, initialized = false;
  int family_enum = -1;
  amdAprilTagsHandle detector = nullptr;
  uint32_t width = 0, height = 0;  // the handle's size: the first frame's, or NodeOptions::max_width x max_height
  bool mixed = false;              // max_width and max_height set: streams of any admissible size, batched together (per-frame sizes)
  uint8_t* d_mono = nullptr;       // S mono8 slots
  size_t pitch = 0, slot_bytes = 0;
  void* d_input = nullptr;         // staging for host / colour frames
  size_t d_input_bytes = 0;
  // k: the camera the pose is computed with (NodeOptions::rectify: Knew of `model`, the stream's camera model)
  // dev, pitch: where the staged mono8 frame lies -- the stream's slot of d_mono, or with NodeOptions::resize_width x resize_height,
  // where a frame may be larger than the handle, a buffer of the slot's own (own, own_bytes) that grows with the frames
  struct Slot {
    bool pending = false; Header info_header; std::array<double, 9> k{}; uint32_t width = 0, height = 0; CameraModelEx model;
    uint8_t* dev = nullptr; size_t pitch = 0; void* own = nullptr; size_t own_bytes = 0;
  };
  std::vector<Slot> slots;
  std::vector<std::vector<BundlePose>> last_bundles;   // per stream (NodeOptions::bundles)
  std::vector<std::vector<RigidBundlePose>> last_rigid;   // per stream (NodeOptions::rigid_bundles)
  std::vector<RigBundlePose> last_rig;                 // of the last round (NodeOptions::rig_cameras)

  void Initialize(const CameraInfo& info) {
    if (opt.max_tags <= 0) throw std::runtime_error("'max_tags' must be positive");
    check_camera_options(opt);
    // left over from an attempt that threw after the handle existed (e.g. the slot allocation failed)
    if (detector) { api().destroy(detector); detector = nullptr; }
    if (d_mono) { api().dev_free(d_mono); d_mono = nullptr; }
    amdAprilTagsConfig_t cfg;
    mixed = opt.max_width != 0 && opt.max_height != 0;
    const bool resize = resizing(opt);   // the handle has the size the frames are resized to (mixed: the largest such size)
    api().default_config(&cfg, mixed ? opt.max_width : resize ? opt.resize_width : info.width,
                         mixed ? opt.max_height : resize ? opt.resize_height : info.height);
    cfg.tile_size = opt.tile_size;
    cfg.decimate = opt.decimate;
    cfg.num_families = 1;
    cfg.families[0] = static_cast<amdAprilTagsFamily>(family_enum);
    const std::array<double, 9> k = pose_camera(opt, info);
    cfg.intrinsics.fx = static_cast<float>(k[0]);
    cfg.intrinsics.fy = static_cast<float>(k[4]);
    cfg.intrinsics.cx = static_cast<float>(k[2]);
    cfg.intrinsics.cy = static_cast<float>(k[5]);
    // (VPI mode passes every camera's own skew K[1], src/apriltag_node.cpp:215-225: set per frame at every flush)
    cfg.skew = cuapriltags_mode ? 0.0f : static_cast<float>(k[1]);
    cfg.tag_size = static_cast<float>(opt.size);
    cfg.max_batch = S;
    const int error = api().create_ex(&detector, &cfg);
    if (error != 0) throw std::runtime_error("Failed to create AprilTags detector (error code " + std::to_string(error) + ")");
    apply_quad_sigma(detector, opt.quad_sigma);
    if (mixed && api().set_per_frame_sizes(detector, 1) != 0) throw std::runtime_error("per-frame image sizes refused");
    apply_resize(detector, opt);
    apply_bundles(detector, opt);
    apply_rigid_bundles(detector, opt);
    apply_tag_table(detector, opt);
    apply_pose_refinement(detector, opt);
    apply_pose_covariance(detector, opt);
    apply_rig(detector, opt, S);
    width = cfg.width;
    height = cfg.height;
    pitch = (static_cast<size_t>(width) + 63) & ~static_cast<size_t>(63);
    slot_bytes = pitch * height;
    if (!resize) {   // (resize: every slot stages into a buffer of its own, sized by its frames)
      void* p = nullptr;
      if (api().dev_alloc(&p, slot_bytes * S) != 0) throw std::runtime_error("device allocation failed");
      d_mono = static_cast<uint8_t*>(p);
    }
    initialized = true;
  }

  // the frame of `stream` ends up as mono8 in its device slot
  bool Stage(uint32_t stream, const Image& image, const CameraInfo& info) {
    const int bpp = bytes_per_pixel(image.encoding);
    if (bpp == 0) {
      std::fprintf(stderr, "[apriltag_node] Unsupported image encoding: %s\n", image.encoding.c_str());
      throw std::runtime_error("AprilTags detector only supports 'mono8', 'rgb8', 'bgr8', 'rgba8' or 'bgra8' image input");
    }
    // one size (the first frame's), or -- max_width x max_height set -- every size the handle admits (include/apriltag_amd.h,
    // amdAprilTagsSetPerFrameSizes: up to the handle's, a full threshold tile of the working image in both directions)
    const auto working = [&](uint32_t v) { return 1 + (v - 1) / opt.decimate; };
    const bool resize = resizing(opt);
    const bool size_ok = resize ? image.width >= 1 && image.width <= 16384 && image.height >= 1 && image.height <= 16384
                         : mixed ? image.width >= 1 && image.width <= width && image.height >= 1 && image.height <= height &&
                                     working(image.width) >= opt.tile_size && working(image.height) >= opt.tile_size
                                 : image.width == width && image.height == height;
    if (!size_ok || info.width != image.width || info.height != image.height ||
        static_cast<size_t>(image.step) < static_cast<size_t>(image.width) * bpp || image.data == nullptr) {
      std::fprintf(stderr, "[apriltag_node] stream %u: image %ux%u (step %u) does not match the initialised size %s%ux%u: frame dropped\n",
                   stream, image.width, image.height, image.step, mixed ? "up to " : "", width, height);
      return false;
    }
    slots[stream].width = image.width;
    slots[stream].height = image.height;
    const uint8_t* dev_src = image.data;
    Slot& sl = slots[stream];
    if (resize) {
      sl.pitch = (static_cast<size_t>(image.width) + 63) & ~static_cast<size_t>(63);
      const size_t need = sl.pitch * image.height;
      if (need > sl.own_bytes) {
        if (sl.own) api().dev_free(sl.own);
        sl.own = nullptr; sl.own_bytes = 0;
        if (api().dev_alloc(&sl.own, need) != 0) throw std::runtime_error("device allocation failed");
        sl.own_bytes = need;
      }
      sl.dev = static_cast<uint8_t*>(sl.own);
    } else {
      sl.dev = d_mono + slot_bytes * stream;
      sl.pitch = this->pitch;
    }
    uint8_t* slot = sl.dev;
    const size_t pitch = sl.pitch;
    if (!image.is_device) {
      const size_t bytes = static_cast<size_t>(image.step) * image.height;
      if (bpp == 1 && image.step == pitch) {   // straight into the slot
        if (api().copy_to_device(slot, image.data, bytes, nullptr) != 0) return false;
        return true;
      }
      if (bytes > d_input_bytes) {
        if (d_input) api().dev_free(d_input);
        d_input = nullptr;
        if (api().dev_alloc(&d_input, bytes) != 0) throw std::runtime_error("device allocation failed");
        d_input_bytes = bytes;
      }
      if (api().copy_to_device(d_input, image.data, bytes, nullptr) != 0) return false;
      dev_src = static_cast<const uint8_t*>(d_input);
    }
    // mono8 with another pitch is repacked by the conversion entry point as well (one 8-bit channel in, one out)
    return api().to_mono8(dev_src, image.step, image.encoding.c_str(), image.width, image.height, slot, pitch, nullptr) == 0;
  }
};

AprilTagMultiCameraNode::AprilTagMultiCameraNode(const NodeOptions& options, uint32_t num_streams) : impl_(new Impl()) {
  if (num_streams == 0 || num_streams > 65535) throw std::runtime_error("'num_streams' must be 1..65535");
  impl_->opt = options;
  impl_->S = num_streams;
  impl_->slots.resize(num_streams);
  impl_->last_bundles.resize(num_streams);
  impl_->last_rigid.resize(num_streams);
  impl_->family_enum = validate_family(options, &impl_->cuapriltags_mode);
  check_tags(options);
}

AprilTagMultiCameraNode::~AprilTagMultiCameraNode() {
  if (impl_) {
    if (impl_->detector) api().destroy(impl_->detector);
    if (impl_->d_input) api().dev_free(impl_->d_input);
    if (impl_->d_mono) api().dev_free(impl_->d_mono);
    for (auto& sl : impl_->slots) if (sl.own) api().dev_free(sl.own);
  }
}

void AprilTagMultiCameraNode::set_detections_callback(DetectionsCallback cb) { impl_->on_detections = std::move(cb); }
void AprilTagMultiCameraNode::set_transforms_callback(TransformsCallback cb) { impl_->on_transforms = std::move(cb); }
void AprilTagMultiCameraNode::set_auto_flush(bool on) { impl_->auto_flush = on; }
uint32_t AprilTagMultiCameraNode::num_streams() const { return impl_->S; }
const std::vector<BundlePose>& AprilTagMultiCameraNode::last_bundle_poses(uint32_t stream) const { return impl_->last_bundles.at(stream); }
const std::vector<RigidBundlePose>& AprilTagMultiCameraNode::last_rigid_bundle_poses(uint32_t stream) const { return impl_->last_rigid.at(stream); }
const std::vector<RigBundlePose>& AprilTagMultiCameraNode::last_rig_bundle_poses() const { return impl_->last_rig; }
const NodeOptions& AprilTagMultiCameraNode::options() const { return impl_->opt; }

bool AprilTagMultiCameraNode::CameraImageCallback(uint32_t stream, const Image& image, const CameraInfo& camera_info) {
  if (stream >= impl_->S) throw std::runtime_error("stream index out of range");
  if (image.header.stamp.sec != camera_info.header.stamp.sec || image.header.stamp.nanosec != camera_info.header.stamp.nanosec)
    return false;  // ExactTime synchroniser would not fire
  CameraModelEx model;
  if (rectifying(impl_->opt)) model = stream_model(impl_->opt, camera_info);   // (throws before anything is staged)
  if (undistorting(impl_->opt)) model = detected_model(impl_->opt, camera_info);
  if (!impl_->initialized) impl_->Initialize(camera_info);
  Impl::Slot& sl = impl_->slots[stream];
  // the slot's device image is about to be overwritten: a frame staged earlier and not yet submitted is gone either way,
  // and a failed staging must not leave it pending under its old header
  sl.pending = false;
  if (!impl_->Stage(stream, image, camera_info)) return false;
  sl.pending = true;
  sl.info_header = camera_info.header;
  sl.k = pose_camera(impl_->opt, camera_info);   // (rectify: Knew; resize: scaled to the resized image)
  sl.model = model;
  if (impl_->auto_flush) {
    bool all = true;
    for (const auto& x : impl_->slots) all &= x.pending;
    if (all) Flush();
  }
  return true;
}

uint32_t AprilTagMultiCameraNode::Flush() {
  Impl& I = *impl_;
  std::vector<uint32_t> who;
  for (uint32_t s = 0; s < I.S; s++) if (I.slots[s].pending) who.push_back(s);
  if (who.empty() || !I.initialized) return 0;
  const uint32_t n = static_cast<uint32_t>(who.size());
  std::vector<amdAprilTagsImageInput_t> imgs(n);
  std::vector<amdAprilTagsCameraIntrinsics_t> intr(n);
  for (uint32_t i = 0; i < n; i++) {
    const Impl::Slot& sl = I.slots[who[i]];
    imgs[i].width = sl.width; imgs[i].height = sl.height; imgs[i].dev_ptr = sl.dev; imgs[i].pitch = sl.pitch;
    // K of the stream's own CameraInfo, double -> float as the reference does (src/apriltag_node.cpp:442-447)
    intr[i].fx = static_cast<float>(sl.k[0]); intr[i].fy = static_cast<float>(sl.k[4]);
    intr[i].cx = static_cast<float>(sl.k[2]); intr[i].cy = static_cast<float>(sl.k[5]);
  }
  const uint32_t max_tags = static_cast<uint32_t>(I.opt.max_tags);
  std::vector<amdAprilTagsID_t> tags(static_cast<size_t>(n) * max_tags);
  std::vector<uint32_t> counts(n, 0);
  if (!I.cuapriltags_mode) {   // every stream's own K[1], as S independent VPI-mode nodes would pass it
    std::vector<float> skews(n);
    for (uint32_t i = 0; i < n; i++) skews[i] = static_cast<float>(I.slots[who[i]].k[1]);
    if (api().set_frame_skews(I.detector, n, skews.data()) != 0) {   // (a round whose skews were refused must not run with stale ones)
      std::fprintf(stderr, "[apriltag_node] per-stream skews refused: round dropped\n");
      for (uint32_t s : who) I.slots[s].pending = false;
      return 0;
    }
  }
  if (rectifying(I.opt)) {   // the models of the streams of this round, in slot order (host state of the handle: no device work)
    std::vector<CameraModelEx> models(n);
    for (uint32_t i = 0; i < n; i++) models[i] = I.slots[who[i]].model;
    const int rerr = apply_models(I.detector, I.opt, models.data(), n);
    if (rerr != 0) {   // (a round whose models were refused must not run with stale ones)
      std::fprintf(stderr, "[apriltag_node] per-stream camera models refused (error code %d): round dropped\n", rerr);
      for (uint32_t s : who) I.slots[s].pending = false;
      return 0;
    }
  }
  if (undistorting(I.opt)) {   // raw-frame mode: the same, for the corner undistortion
    std::vector<CameraModelEx> models(n);
    for (uint32_t i = 0; i < n; i++) models[i] = I.slots[who[i]].model;
    const int rerr = apply_corner_models(I.detector, models.data(), n);
    if (rerr != 0) {
      std::fprintf(stderr, "[apriltag_node] per-stream camera models refused (error code %d): round dropped\n", rerr);
      for (uint32_t s : who) I.slots[s].pending = false;
      return 0;
    }
  }
  if (!I.opt.rig_cameras.empty()) {   // one instant: every served stream is its own camera of group 0 (host state of the handle)
    std::vector<amdAprilTagsRigSlot_t> rig_slots(n);
    for (uint32_t i = 0; i < n; i++) rig_slots[i] = {0u, who[i]};
    if (api().set_rig_slots(I.detector, n, rig_slots.data()) != 0) {   // (a round whose slot map was refused must not run with a stale one)
      std::fprintf(stderr, "[apriltag_node] rig slot map refused: round dropped\n");
      for (uint32_t s : who) I.slots[s].pending = false;
      return 0;
    }
  }
  const int error = api().detect_batch(I.detector, n, imgs.data(), intr.data(), tags.data(), counts.data(), max_tags, nullptr);
  for (uint32_t s : who) I.slots[s].pending = false;
  if (error != 0) {
    // the reference logs and drops the frame (src/apriltag_node.cpp:494-497); here: the round
    std::fprintf(stderr, "[apriltag_node] Failed to run AprilTags detector (error code %d)\n", error);
    return 0;
  }
  std::vector<AprilTagDetectionArray> msgs(n);
  std::vector<std::vector<TransformStamped>> tfs(n);
  std::vector<const Header*> headers(n);
  std::vector<std::vector<TransformStamped>*> tf_ptrs(n);
  for (uint32_t i = 0; i < n; i++) {
    std::vector<uint8_t> invalid;
    if (!undistort_tags(I.detector, I.opt, i, tags.data() + static_cast<size_t>(i) * max_tags, counts[i], &invalid)) {
      std::fprintf(stderr, "[apriltag_node] undistorted detections not available: round dropped\n");
      return 0;
    }
    std::vector<std::array<double, 36>> covs;
    if (!refine_tags(I.detector, I.opt, i, tags.data() + static_cast<size_t>(i) * max_tags, counts[i], &covs, invalid)) {
      std::fprintf(stderr, "[apriltag_node] refined poses or their covariances not available: round dropped\n");
      return 0;
    }
    assemble_messages(tags.data() + static_cast<size_t>(i) * max_tags, counts[i], I.slots[who[i]].info_header, I.opt, &msgs[i], &tfs[i],
                      &covs);
    headers[i] = &I.slots[who[i]].info_header;
    tf_ptrs[i] = &tfs[i];
  }
  std::vector<std::vector<BundlePose>> poses;
  if (!collect_bundles(I.detector, I.opt, n, headers.data(), &poses, tf_ptrs.data())) {
    std::fprintf(stderr, "[apriltag_node] bundle records not available: round dropped\n");
    return 0;
  }
  std::vector<std::vector<RigidBundlePose>> rigid;
  if (!collect_rigid_bundles(I.detector, I.opt, n, headers.data(), &rigid, tf_ptrs.data())) {
    std::fprintf(stderr, "[apriltag_node] rigid bundle records not available: round dropped\n");
    return 0;
  }
  std::vector<RigBundlePose> rig;
  if (!collect_rig_bundles(I.detector, I.opt, who, *headers[0], &rig, tf_ptrs[0])) {
    std::fprintf(stderr, "[apriltag_node] rig bundle records not available: round dropped\n");
    return 0;
  }
  I.last_rig = rig;
  for (uint32_t i = 0; i < n; i++) {
    I.last_bundles[who[i]] = poses[i];
    I.last_rigid[who[i]] = rigid[i];
    if (I.on_detections) I.on_detections(who[i], msgs[i]);
    if (I.on_transforms) I.on_transforms(who[i], tfs[i]);
  }
  return n;
}

}  // namespace apriltag
}  // namespace isaac_ros
}  // namespace amd

// ---- flat C view of the shell for the Python test harness (tests/test_node_shell_*.py) ---------------
using amd::isaac_ros::apriltag::AprilTagDetectionArray;
using amd::isaac_ros::apriltag::AprilTagNode;
using amd::isaac_ros::apriltag::CameraInfo;
using amd::isaac_ros::apriltag::Image;
using amd::isaac_ros::apriltag::NodeOptions;
using amd::isaac_ros::apriltag::TransformStamped;

struct NodeShellHarness {
  std::unique_ptr<AprilTagNode> node;
  AprilTagDetectionArray last;
  std::vector<TransformStamped> last_tf;
  int publishes = 0;
  bool is_bigendian = false;   // node_shell_set_bigendian
};

struct NodeShellDetection {
  int32_t id;
  char family[32];
  double center[2];
  double corners[4][2];
  double position[3];
  double orientation_xyzw[4];
  char child_frame_id[48];
};

extern "C" {

// sensor_msgs/CameraInfo's D, distortion_model and P through the flat view (null / 0: left empty)
static void fill_camera_info_extras(CameraInfo* info, const double* d, int nd, const char* distortion_model, const double* p12,
                                    const double* r9 = nullptr) {
  if (d && nd > 0) info->d.assign(d, d + nd);
  if (distortion_model) info->distortion_model = distortion_model;
  if (p12) for (int i = 0; i < 12; i++) info->p[i] = p12[i];
  if (r9) for (int i = 0; i < 9; i++) info->r[i] = r9[i];
}

// the flat value of `rectify`: 0 off, 1 NodeOptions::rectify, 2 NodeOptions::rectify_full, 3 NodeOptions::undistort_corners
static void set_rectify_option(NodeOptions* o, int rectify) {
  o->rectify = rectify == 1;
  o->rectify_full = rectify == 2;
  o->undistort_corners = rectify == 3;
}

// RectificationModelEx of a CameraInfo with these fields: out36 = kind, K[9], D[8], R[9], Knew[9].  0, or -2 with the exception's text.
// (host only: loads no detector library)
int node_shell_camera_model_ex(const double* k9, const double* d, int nd, const char* distortion_model, const double* p12,
                               const double* r9, double* out36, char* err, size_t err_len) {
  try {
    CameraInfo info;
    for (int i = 0; i < 9; i++) info.k[i] = k9[i];
    fill_camera_info_extras(&info, d, nd, distortion_model, p12, r9);
    const amd::isaac_ros::apriltag::CameraModelEx m = amd::isaac_ros::apriltag::RectificationModelEx(info);
    out36[0] = static_cast<double>(m.kind);
    for (int i = 0; i < 9; i++) { out36[1 + i] = m.k[i]; out36[18 + i] = m.r[i]; out36[27 + i] = m.knew[i]; }
    for (int i = 0; i < 8; i++) out36[10 + i] = m.d[i];
    return 0;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return -2;
  }
}

// RectificationModel of a CameraInfo with these fields: out23 = K[9], D[5], Knew[9].  0, or -2 with the exception's text in err.
// (host only: loads no detector library)
int node_shell_camera_model(const double* k9, const double* d, int nd, const char* distortion_model, const double* p12, double* out23,
                            char* err, size_t err_len) {
  try {
    CameraInfo info;
    for (int i = 0; i < 9; i++) info.k[i] = k9[i];
    fill_camera_info_extras(&info, d, nd, distortion_model, p12);
    const amd::isaac_ros::apriltag::CameraModel m = amd::isaac_ros::apriltag::RectificationModel(info);
    for (int i = 0; i < 9; i++) { out23[i] = m.k[i]; out23[14 + i] = m.knew[i]; }
    for (int i = 0; i < 5; i++) out23[9 + i] = m.d[i];
    return 0;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return -2;
  }
}

// Every NodeOptions field the flat view carries (node.py): the create calls below are this one with quad_sigma 0, rectify off and no resize.
NodeShellHarness* node_shell_create_opts(int max_tags, double size, int tile_size, const char* tag_family, const char* backends,
                                         int decimate, int strict_cuapriltags_encodings, double quad_sigma, int rectify,
                                         uint32_t resize_width, uint32_t resize_height, char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    o.strict_cuapriltags_encodings = strict_cuapriltags_encodings != 0;
    o.quad_sigma = quad_sigma;
    set_rectify_option(&o, rectify);
    o.resize_width = resize_width; o.resize_height = resize_height;
    auto* h = new NodeShellHarness();
    h->node.reset(new AprilTagNode(o));
    h->node->set_detections_callback([h](const AprilTagDetectionArray& m) { h->last = m; h->publishes++; });
    h->node->set_transforms_callback([h](const std::vector<TransformStamped>& t) { h->last_tf = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}

// NodeOptions::raw_shift through the flat view, beside the options of node_shell_create_ex
NodeShellHarness* node_shell_create_raw(int max_tags, double size, int tile_size, const char* tag_family, const char* backends,
                                        int decimate, int strict_cuapriltags_encodings, uint32_t raw_shift, char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    o.strict_cuapriltags_encodings = strict_cuapriltags_encodings != 0;
    o.raw_shift = raw_shift;
    auto* h = new NodeShellHarness();
    h->node.reset(new AprilTagNode(o));
    h->node->set_detections_callback([h](const AprilTagDetectionArray& m) { h->last = m; h->publishes++; });
    h->node->set_transforms_callback([h](const std::vector<TransformStamped>& t) { h->last_tf = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}
// sensor_msgs/Image.is_bigendian of the frames fed from here on (node_shell_on_frame and its kin keep their signatures)
void node_shell_set_bigendian(NodeShellHarness* h, int is_bigendian) { h->is_bigendian = is_bigendian != 0; }

NodeShellHarness* node_shell_create_ex(int max_tags, double size, int tile_size, const char* tag_family, const char* backends,
                                       int decimate, int strict_cuapriltags_encodings, double quad_sigma, char* err, size_t err_len) {
  return node_shell_create_opts(max_tags, size, tile_size, tag_family, backends, decimate, strict_cuapriltags_encodings, quad_sigma, 0,
                                0, 0, err, err_len);
}

// Returns nullptr and fills err on a constructor exception (mirrors test/apriltag_node_test.cpp).
NodeShellHarness* node_shell_create(int max_tags, double size, int tile_size, const char* tag_family, const char* backends,
                                    int decimate, char* err, size_t err_len) {
  return node_shell_create_ex(max_tags, size, tile_size, tag_family, backends, decimate, 0, 0.0, err, err_len);
}

// the same with NodeOptions::strict_cuapriltags_encodings set
NodeShellHarness* node_shell_create_strict(int max_tags, double size, int tile_size, const char* tag_family, const char* backends,
                                           int decimate, char* err, size_t err_len) {
  return node_shell_create_ex(max_tags, size, tile_size, tag_family, backends, decimate, 1, 0.0, err, err_len);
}

// NodeOptions::bundles through the flat view: members holds four doubles per member -- id, x, y, size
struct NodeShellBundle {
  char name[32];
  const double* members;
  uint32_t nmembers, max_hamming, min_tags, pad;
  double min_decision_margin;
};
struct NodeShellTransform {
  char child_frame_id[48];
  char frame_id[48];
  int32_t sec;
  uint32_t nanosec;
  double translation[3];
  double rotation_xyzw[4];
};
struct NodeShellBundlePose {
  char name[32];
  uint32_t status, ntags, nskipped, pad;
  double R[9], t[3], sq_err_sum;
};

static void set_bundle_options(NodeOptions* o, int nbundles, const NodeShellBundle* bundles) {
  for (int b = 0; b < nbundles; b++) {
    amd::isaac_ros::apriltag::Bundle out;
    out.name = std::string(bundles[b].name, strnlen(bundles[b].name, sizeof(bundles[b].name)));
    for (uint32_t m = 0; m < bundles[b].nmembers; m++) {
      const double* v = bundles[b].members + 4 * m;
      out.members.push_back({static_cast<uint32_t>(v[0]), v[1], v[2], v[3]});
    }
    out.max_hamming = bundles[b].max_hamming; out.min_tags = bundles[b].min_tags; out.min_decision_margin = bundles[b].min_decision_margin;
    o->bundles.push_back(out);
  }
}
// NodeOptions::rigid_bundles through the flat view: members holds nine doubles per member -- id, x, y, z, qw, qx, qy, qz, size
struct NodeShellRigidBundle {
  char name[32];
  const double* members;
  uint32_t nmembers, max_hamming, min_tags, iterations;
  double min_decision_margin;
};
struct NodeShellRigidBundlePose {
  char name[32];
  uint32_t status, ntags, nskipped, seed, chosen, pad;
  double R[9], t[3], err, sq_err_sum, R_alt[9], t_alt[3], err_alt, sq_err_sum_alt;
};
static void set_rigid_bundle_options(NodeOptions* o, int nbundles, const NodeShellRigidBundle* bundles) {
  for (int b = 0; b < nbundles; b++) {
    amd::isaac_ros::apriltag::RigidBundle out;
    out.name = std::string(bundles[b].name, strnlen(bundles[b].name, sizeof(bundles[b].name)));
    for (uint32_t m = 0; m < bundles[b].nmembers; m++) {
      const double* v = bundles[b].members + 9 * m;
      out.members.push_back({static_cast<uint32_t>(v[0]), v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]});
    }
    out.max_hamming = bundles[b].max_hamming; out.min_tags = bundles[b].min_tags; out.min_decision_margin = bundles[b].min_decision_margin;
    out.iterations = bundles[b].iterations;
    o->rigid_bundles.push_back(out);
  }
}
static int copy_rigid_bundle_poses(const std::vector<amd::isaac_ros::apriltag::RigidBundlePose>& poses, NodeShellRigidBundlePose* out, int max_out) {
  const int n = static_cast<int>(poses.size());
  for (int i = 0; i < n && i < max_out; i++) {
    NodeShellRigidBundlePose& o = out[i];
    std::memset(&o, 0, sizeof(o));
    std::strncpy(o.name, poses[i].name.c_str(), sizeof(o.name) - 1);
    o.status = poses[i].status; o.ntags = poses[i].ntags; o.nskipped = poses[i].nskipped; o.seed = poses[i].seed; o.chosen = poses[i].chosen;
    o.err = poses[i].err; o.sq_err_sum = poses[i].sq_err_sum; o.err_alt = poses[i].err_alt; o.sq_err_sum_alt = poses[i].sq_err_sum_alt;
    for (int k = 0; k < 9; k++) { o.R[k] = poses[i].R[k]; o.R_alt[k] = poses[i].R_alt[k]; }
    for (int k = 0; k < 3; k++) { o.t[k] = poses[i].t[k]; o.t_alt[k] = poses[i].t_alt[k]; }
  }
  return n;
}
static int copy_transforms(const std::vector<TransformStamped>& tfs, NodeShellTransform* out, int max_out) {
  const int n = static_cast<int>(tfs.size());
  for (int i = 0; i < n && i < max_out; i++) {
    NodeShellTransform& o = out[i];
    std::memset(&o, 0, sizeof(o));
    std::strncpy(o.child_frame_id, tfs[i].child_frame_id.c_str(), sizeof(o.child_frame_id) - 1);
    std::strncpy(o.frame_id, tfs[i].header.frame_id.c_str(), sizeof(o.frame_id) - 1);
    o.sec = tfs[i].header.stamp.sec; o.nanosec = tfs[i].header.stamp.nanosec;
    o.translation[0] = tfs[i].transform.translation.x; o.translation[1] = tfs[i].transform.translation.y; o.translation[2] = tfs[i].transform.translation.z;
    o.rotation_xyzw[0] = tfs[i].transform.rotation.x; o.rotation_xyzw[1] = tfs[i].transform.rotation.y;
    o.rotation_xyzw[2] = tfs[i].transform.rotation.z; o.rotation_xyzw[3] = tfs[i].transform.rotation.w;
  }
  return n;
}
static int copy_bundle_poses(const std::vector<amd::isaac_ros::apriltag::BundlePose>& poses, NodeShellBundlePose* out, int max_out) {
  const int n = static_cast<int>(poses.size());
  for (int i = 0; i < n && i < max_out; i++) {
    NodeShellBundlePose& o = out[i];
    std::memset(&o, 0, sizeof(o));
    std::strncpy(o.name, poses[i].name.c_str(), sizeof(o.name) - 1);
    o.status = poses[i].status; o.ntags = poses[i].ntags; o.nskipped = poses[i].nskipped; o.sq_err_sum = poses[i].sq_err_sum;
    for (int k = 0; k < 9; k++) o.R[k] = poses[i].R[k];
    for (int k = 0; k < 3; k++) o.t[k] = poses[i].t[k];
  }
  return n;
}

// AprilTagNode with NodeOptions::bundles (the other options at their defaults but those named)
NodeShellHarness* node_shell_create_bundles(int max_tags, double size, int tile_size, const char* tag_family, const char* backends,
                                            int decimate, int nbundles, const NodeShellBundle* bundles, char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    set_bundle_options(&o, nbundles, bundles);
    auto* h = new NodeShellHarness();
    h->node.reset(new AprilTagNode(o));
    h->node->set_detections_callback([h](const AprilTagDetectionArray& m) { h->last = m; h->publishes++; });
    h->node->set_transforms_callback([h](const std::vector<TransformStamped>& t) { h->last_tf = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}
// AprilTagNode with NodeOptions::rigid_bundles (the other options at their defaults but those named)
NodeShellHarness* node_shell_create_rigid_bundles(int max_tags, double size, int tile_size, const char* tag_family, const char* backends,
                                                  int decimate, int nbundles, const NodeShellRigidBundle* bundles, char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    set_rigid_bundle_options(&o, nbundles, bundles);
    auto* h = new NodeShellHarness();
    h->node.reset(new AprilTagNode(o));
    h->node->set_detections_callback([h](const AprilTagDetectionArray& m) { h->last = m; h->publishes++; });
    h->node->set_transforms_callback([h](const std::vector<TransformStamped>& t) { h->last_tf = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}
int node_shell_last_rigid_bundle_poses(NodeShellHarness* h, NodeShellRigidBundlePose* out, int max_out) {
  return copy_rigid_bundle_poses(h->node->last_rigid_bundle_poses(), out, max_out);
}
// AprilTagNode with NodeOptions::pose_refinement (the other options at their defaults but those named)
NodeShellHarness* node_shell_create_refined(int max_tags, double size, int tile_size, const char* tag_family, const char* backends,
                                            int decimate, uint32_t pose_refinement, char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    o.pose_refinement = pose_refinement;
    auto* h = new NodeShellHarness();
    h->node.reset(new AprilTagNode(o));
    h->node->set_detections_callback([h](const AprilTagDetectionArray& m) { h->last = m; h->publishes++; });
    h->node->set_transforms_callback([h](const std::vector<TransformStamped>& t) { h->last_tf = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}
// NodeOptions::tags through the flat view: ntags entries, frame "" for none (the field is wider than the 47 characters a frame may
// have, so that a frame too long reaches the constructor and is refused there)
struct NodeShellTag {
  uint32_t id;
  double size;
  char frame[64];
};
static void flat_tags(NodeOptions* o, int ntags, const NodeShellTag* tags, int listed_only) {
  for (int i = 0; i < ntags; i++) {
    amd::isaac_ros::apriltag::TagSpec t;
    t.id = tags[i].id; t.size = tags[i].size;
    t.frame = std::string(tags[i].frame, strnlen(tags[i].frame, sizeof(tags[i].frame)));
    o->tags.push_back(t);
  }
  o->tags_listed_only = listed_only != 0;
}
// AprilTagNode with NodeOptions::tags / tags_listed_only beside pose_refinement (0: off)
NodeShellHarness* node_shell_create_tags(int max_tags, double size, int tile_size, const char* tag_family, const char* backends,
                                         int decimate, uint32_t pose_refinement, int ntags, const NodeShellTag* tags,
                                         int listed_only, char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    o.pose_refinement = pose_refinement;
    flat_tags(&o, ntags, tags, listed_only);
    auto* h = new NodeShellHarness();
    h->node.reset(new AprilTagNode(o));
    h->node->set_detections_callback([h](const AprilTagDetectionArray& m) { h->last = m; h->publishes++; });
    h->node->set_transforms_callback([h](const std::vector<TransformStamped>& t) { h->last_tf = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}
// AprilTagNode with NodeOptions::undistort_corners beside pose_refinement (and pose_covariance_sigma_px; 0: off)
NodeShellHarness* node_shell_create_undistort_refined(int max_tags, double size, int tile_size, const char* tag_family, const char* backends,
                                                      int decimate, uint32_t pose_refinement, double sigma_px, char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    o.pose_refinement = pose_refinement;
    o.pose_covariance_sigma_px = sigma_px;
    o.undistort_corners = true;
    auto* h = new NodeShellHarness();
    h->node.reset(new AprilTagNode(o));
    h->node->set_detections_callback([h](const AprilTagDetectionArray& m) { h->last = m; h->publishes++; });
    h->node->set_transforms_callback([h](const std::vector<TransformStamped>& t) { h->last_tf = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}
// AprilTagNode with NodeOptions::pose_covariance_sigma_px beside pose_refinement and / or rigid_bundles (nbundles 0: none)
NodeShellHarness* node_shell_create_covariance(int max_tags, double size, int tile_size, const char* tag_family, const char* backends,
                                               int decimate, uint32_t pose_refinement, int nbundles, const NodeShellRigidBundle* bundles,
                                               double pose_covariance_sigma_px, char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    o.pose_refinement = pose_refinement;
    set_rigid_bundle_options(&o, nbundles, bundles);
    o.pose_covariance_sigma_px = pose_covariance_sigma_px;
    auto* h = new NodeShellHarness();
    h->node.reset(new AprilTagNode(o));
    h->node->set_detections_callback([h](const AprilTagDetectionArray& m) { h->last = m; h->publishes++; });
    h->node->set_transforms_callback([h](const std::vector<TransformStamped>& t) { h->last_tf = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}
// detection.pose.pose.covariance of the last published message, 36 doubles per detection; the number of detections
static int copy_covariances(const AprilTagDetectionArray& m, double* out36, int max_out) {
  const int n = static_cast<int>(m.detections.size());
  for (int i = 0; i < n && i < max_out; i++)
    for (int k = 0; k < 36; k++) out36[36 * i + k] = m.detections[i].pose.pose.covariance[k];
  return n;
}
static int copy_rigid_covariances(const std::vector<amd::isaac_ros::apriltag::RigidBundlePose>& poses, double* out36, int max_out) {
  const int n = static_cast<int>(poses.size());
  for (int i = 0; i < n && i < max_out; i++)
    for (int k = 0; k < 36; k++) out36[36 * i + k] = poses[i].covariance[k];
  return n;
}
int node_shell_last_covariances(NodeShellHarness* h, double* out36, int max_out) { return copy_covariances(h->last, out36, max_out); }
int node_shell_last_rigid_covariances(NodeShellHarness* h, double* out36, int max_out) {
  return copy_rigid_covariances(h->node->last_rigid_bundle_poses(), out36, max_out);
}
// the transforms of the last published frame (tags first, then one per solved bundle), and its bundle records
int node_shell_last_transforms(NodeShellHarness* h, NodeShellTransform* out, int max_out) { return copy_transforms(h->last_tf, out, max_out); }
int node_shell_last_bundle_poses(NodeShellHarness* h, NodeShellBundlePose* out, int max_out) {
  return copy_bundle_poses(h->node->last_bundle_poses(), out, max_out);
}

void node_shell_destroy(NodeShellHarness* h) { delete h; }

// Feeds one image + camera_info pair.  Returns the number of detections published, -1 if the stamps
// differ (no callback), -2 on an exception (message in err).
// (d, nd, distortion_model, p12, r9: the CameraInfo fields NodeOptions::rectify and rectify_full read)
int node_shell_on_frame_full(NodeShellHarness* h, const uint8_t* data, int is_device, const char* encoding, uint32_t width,
                             uint32_t height, uint32_t step, const double* k9, const double* d, int nd, const char* distortion_model,
                             const double* p12, const double* r9, const char* frame_id, int32_t sec, uint32_t nanosec, int32_t info_sec,
                             uint32_t info_nanosec, NodeShellDetection* out, int max_out, char* out_frame_id, size_t frame_id_len,
                             char* err, size_t err_len) {
  try {
    Image img;
    img.header.frame_id = "image_frame"; img.header.stamp.sec = sec; img.header.stamp.nanosec = nanosec;
    img.width = width; img.height = height; img.step = step; img.encoding = encoding; img.data = data; img.is_device = is_device != 0;
    img.is_bigendian = h->is_bigendian;
    CameraInfo info;
    info.header.frame_id = frame_id; info.header.stamp.sec = info_sec; info.header.stamp.nanosec = info_nanosec;
    info.width = width; info.height = height;
    for (int i = 0; i < 9; i++) info.k[i] = k9[i];
    fill_camera_info_extras(&info, d, nd, distortion_model, p12, r9);
    const int before = h->publishes;
    if (!h->node->CameraImageCallback(img, info)) return -1;
    if (h->publishes == before) return 0;  // frame dropped
    const auto& m = h->last;
    if (out_frame_id && frame_id_len) { std::strncpy(out_frame_id, m.header.frame_id.c_str(), frame_id_len - 1); out_frame_id[frame_id_len - 1] = 0; }
    int n = static_cast<int>(m.detections.size());
    for (int i = 0; i < n && i < max_out; i++) {
      const auto& d = m.detections[i];
      NodeShellDetection& o = out[i];
      std::memset(&o, 0, sizeof(o));
      o.id = d.id;
      std::strncpy(o.family, d.family.c_str(), sizeof(o.family) - 1);
      o.center[0] = d.center.x; o.center[1] = d.center.y;
      for (int c = 0; c < 4; c++) { o.corners[c][0] = d.corners[c].x; o.corners[c][1] = d.corners[c].y; }
      o.position[0] = d.pose.pose.pose.position.x; o.position[1] = d.pose.pose.pose.position.y; o.position[2] = d.pose.pose.pose.position.z;
      o.orientation_xyzw[0] = d.pose.pose.pose.orientation.x; o.orientation_xyzw[1] = d.pose.pose.pose.orientation.y;
      o.orientation_xyzw[2] = d.pose.pose.pose.orientation.z; o.orientation_xyzw[3] = d.pose.pose.pose.orientation.w;
      std::strncpy(o.child_frame_id, h->last_tf[i].child_frame_id.c_str(), sizeof(o.child_frame_id) - 1);
    }
    return n;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return -2;
  }
}

int node_shell_on_frame_info(NodeShellHarness* h, const uint8_t* data, int is_device, const char* encoding, uint32_t width,
                             uint32_t height, uint32_t step, const double* k9, const double* d, int nd, const char* distortion_model,
                             const double* p12, const char* frame_id, int32_t sec, uint32_t nanosec, int32_t info_sec,
                             uint32_t info_nanosec, NodeShellDetection* out, int max_out, char* out_frame_id, size_t frame_id_len,
                             char* err, size_t err_len) {
  return node_shell_on_frame_full(h, data, is_device, encoding, width, height, step, k9, d, nd, distortion_model, p12, nullptr, frame_id,
                                  sec, nanosec, info_sec, info_nanosec, out, max_out, out_frame_id, frame_id_len, err, err_len);
}

int node_shell_on_frame(NodeShellHarness* h, const uint8_t* data, int is_device, const char* encoding, uint32_t width,
                        uint32_t height, uint32_t step, const double* k9, const char* frame_id, int32_t sec, uint32_t nanosec,
                        int32_t info_sec, uint32_t info_nanosec, NodeShellDetection* out, int max_out, char* out_frame_id,
                        size_t frame_id_len, char* err, size_t err_len) {
  return node_shell_on_frame_info(h, data, is_device, encoding, width, height, step, k9, nullptr, 0, nullptr, nullptr, frame_id, sec,
                                  nanosec, info_sec, info_nanosec, out, max_out, out_frame_id, frame_id_len, err, err_len);
}

// ---- the multi-camera node through the same flat view ----
struct MultiShellHarness {
  std::unique_ptr<amd::isaac_ros::apriltag::AprilTagMultiCameraNode> node;
  std::vector<AprilTagDetectionArray> last;
  std::vector<std::vector<TransformStamped>> last_tf;
  std::vector<int> publishes;
};

// max_width, max_height, rectify, resize_width, resize_height: NodeOptions of the same names (0, 0: one size, the first frame's)
MultiShellHarness* node_shell_multi_create_opts(int num_streams, int max_tags, double size, int tile_size, const char* tag_family,
                                                const char* backends, int decimate, int auto_flush, double quad_sigma,
                                                uint32_t max_width, uint32_t max_height, int rectify, uint32_t resize_width,
                                                uint32_t resize_height, char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    o.quad_sigma = quad_sigma;
    o.max_width = max_width; o.max_height = max_height;
    set_rectify_option(&o, rectify);
    o.resize_width = resize_width; o.resize_height = resize_height;
    auto* h = new MultiShellHarness();
    h->node.reset(new amd::isaac_ros::apriltag::AprilTagMultiCameraNode(o, static_cast<uint32_t>(num_streams)));
    h->node->set_auto_flush(auto_flush != 0);
    h->last.resize(num_streams); h->last_tf.resize(num_streams); h->publishes.assign(num_streams, 0);
    h->node->set_detections_callback([h](uint32_t s, const AprilTagDetectionArray& m) { h->last[s] = m; h->publishes[s]++; });
    h->node->set_transforms_callback([h](uint32_t s, const std::vector<TransformStamped>& t) { h->last_tf[s] = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}

MultiShellHarness* node_shell_multi_create_sized(int num_streams, int max_tags, double size, int tile_size, const char* tag_family,
                                                 const char* backends, int decimate, int auto_flush, double quad_sigma,
                                                 uint32_t max_width, uint32_t max_height, char* err, size_t err_len) {
  return node_shell_multi_create_opts(num_streams, max_tags, size, tile_size, tag_family, backends, decimate, auto_flush, quad_sigma,
                                      max_width, max_height, 0, 0, 0, err, err_len);
}

MultiShellHarness* node_shell_multi_create_ex(int num_streams, int max_tags, double size, int tile_size, const char* tag_family,
                                              const char* backends, int decimate, int auto_flush, double quad_sigma, char* err,
                                              size_t err_len) {
  return node_shell_multi_create_sized(num_streams, max_tags, size, tile_size, tag_family, backends, decimate, auto_flush, quad_sigma, 0, 0,
                                       err, err_len);
}

MultiShellHarness* node_shell_multi_create(int num_streams, int max_tags, double size, int tile_size, const char* tag_family,
                                           const char* backends, int decimate, int auto_flush, char* err, size_t err_len) {
  return node_shell_multi_create_ex(num_streams, max_tags, size, tile_size, tag_family, backends, decimate, auto_flush, 0.0, err, err_len);
}

MultiShellHarness* node_shell_multi_create_bundles(int num_streams, int max_tags, double size, int tile_size, const char* tag_family,
                                                   const char* backends, int decimate, int auto_flush, int nbundles,
                                                   const NodeShellBundle* bundles, char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    set_bundle_options(&o, nbundles, bundles);
    auto* h = new MultiShellHarness();
    h->node.reset(new amd::isaac_ros::apriltag::AprilTagMultiCameraNode(o, static_cast<uint32_t>(num_streams)));
    h->node->set_auto_flush(auto_flush != 0);
    h->last.resize(num_streams); h->last_tf.resize(num_streams); h->publishes.assign(num_streams, 0);
    h->node->set_detections_callback([h](uint32_t s, const AprilTagDetectionArray& m) { h->last[s] = m; h->publishes[s]++; });
    h->node->set_transforms_callback([h](uint32_t s, const std::vector<TransformStamped>& t) { h->last_tf[s] = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}
MultiShellHarness* node_shell_multi_create_rigid_bundles(int num_streams, int max_tags, double size, int tile_size, const char* tag_family,
                                                         const char* backends, int decimate, int auto_flush, int nbundles,
                                                         const NodeShellRigidBundle* bundles, char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    set_rigid_bundle_options(&o, nbundles, bundles);
    auto* h = new MultiShellHarness();
    h->node.reset(new amd::isaac_ros::apriltag::AprilTagMultiCameraNode(o, static_cast<uint32_t>(num_streams)));
    h->node->set_auto_flush(auto_flush != 0);
    h->last.resize(num_streams); h->last_tf.resize(num_streams); h->publishes.assign(num_streams, 0);
    h->node->set_detections_callback([h](uint32_t s, const AprilTagDetectionArray& m) { h->last[s] = m; h->publishes[s]++; });
    h->node->set_transforms_callback([h](uint32_t s, const std::vector<TransformStamped>& t) { h->last_tf[s] = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}
// NodeOptions::rig_cameras through the flat view: twelve doubles per stream -- R row-major, then t -- beside rigid_bundles
struct NodeShellRigBundlePose {
  char name[32];
  uint32_t status, nobs, nskipped, ndropped, ncams, seed_stream, seed, chosen;
  double R[9], t[3], err, sq_err_sum, R_alt[9], t_alt[3], err_alt, sq_err_sum_alt;
};
MultiShellHarness* node_shell_multi_create_rig(int num_streams, int max_tags, double size, int tile_size, const char* tag_family,
                                               const char* backends, int decimate, int auto_flush, int nbundles,
                                               const NodeShellRigidBundle* bundles, int ncams, const double* cams12, const char* rig_frame_id,
                                               char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    set_rigid_bundle_options(&o, nbundles, bundles);
    for (int c = 0; c < ncams; c++) {
      amd::isaac_ros::apriltag::RigCamera cam;
      for (int i = 0; i < 9; i++) cam.R[i] = cams12[12 * c + i];
      for (int i = 0; i < 3; i++) cam.t[i] = cams12[12 * c + 9 + i];
      o.rig_cameras.push_back(cam);
    }
    if (rig_frame_id) o.rig_frame_id = rig_frame_id;
    auto* h = new MultiShellHarness();
    h->node.reset(new amd::isaac_ros::apriltag::AprilTagMultiCameraNode(o, static_cast<uint32_t>(num_streams)));
    h->node->set_auto_flush(auto_flush != 0);
    h->last.resize(num_streams); h->last_tf.resize(num_streams); h->publishes.assign(num_streams, 0);
    h->node->set_detections_callback([h](uint32_t s, const AprilTagDetectionArray& m) { h->last[s] = m; h->publishes[s]++; });
    h->node->set_transforms_callback([h](uint32_t s, const std::vector<TransformStamped>& t) { h->last_tf[s] = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}
int node_shell_multi_last_rig_bundle_poses(MultiShellHarness* h, NodeShellRigBundlePose* out, int max_out) {
  const std::vector<amd::isaac_ros::apriltag::RigBundlePose>& poses = h->node->last_rig_bundle_poses();
  const int n = static_cast<int>(poses.size());
  for (int i = 0; i < n && i < max_out; i++) {
    NodeShellRigBundlePose& o = out[i];
    std::memset(&o, 0, sizeof(o));
    std::strncpy(o.name, poses[i].name.c_str(), sizeof(o.name) - 1);
    o.status = poses[i].status; o.nobs = poses[i].nobs; o.nskipped = poses[i].nskipped; o.ndropped = poses[i].ndropped;
    o.ncams = poses[i].ncams; o.seed_stream = poses[i].seed_stream; o.seed = poses[i].seed; o.chosen = poses[i].chosen;
    for (int k = 0; k < 9; k++) { o.R[k] = poses[i].R[k]; o.R_alt[k] = poses[i].R_alt[k]; }
    for (int k = 0; k < 3; k++) { o.t[k] = poses[i].t[k]; o.t_alt[k] = poses[i].t_alt[k]; }
    o.err = poses[i].err; o.sq_err_sum = poses[i].sq_err_sum; o.err_alt = poses[i].err_alt; o.sq_err_sum_alt = poses[i].sq_err_sum_alt;
  }
  return n;
}
int node_shell_multi_last_rigid_bundle_poses(MultiShellHarness* h, int stream, NodeShellRigidBundlePose* out, int max_out) {
  return copy_rigid_bundle_poses(h->node->last_rigid_bundle_poses(static_cast<uint32_t>(stream)), out, max_out);
}
// AprilTagMultiCameraNode with NodeOptions::undistort_corners beside pose_refinement
MultiShellHarness* node_shell_multi_create_undistort_refined(int num_streams, int max_tags, double size, int tile_size, const char* tag_family,
                                                             const char* backends, int decimate, int auto_flush, uint32_t pose_refinement,
                                                             char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    o.pose_refinement = pose_refinement;
    o.undistort_corners = true;
    auto* h = new MultiShellHarness();
    h->node.reset(new amd::isaac_ros::apriltag::AprilTagMultiCameraNode(o, static_cast<uint32_t>(num_streams)));
    h->node->set_auto_flush(auto_flush != 0);
    h->last.resize(num_streams); h->last_tf.resize(num_streams); h->publishes.assign(num_streams, 0);
    h->node->set_detections_callback([h](uint32_t s, const AprilTagDetectionArray& m) { h->last[s] = m; h->publishes[s]++; });
    h->node->set_transforms_callback([h](uint32_t s, const std::vector<TransformStamped>& t) { h->last_tf[s] = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}
// AprilTagMultiCameraNode with NodeOptions::tags / tags_listed_only beside pose_refinement (0: off)
MultiShellHarness* node_shell_multi_create_tags(int num_streams, int max_tags, double size, int tile_size, const char* tag_family,
                                                const char* backends, int decimate, int auto_flush, uint32_t pose_refinement, int ntags,
                                                const NodeShellTag* tags, int listed_only, char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    o.pose_refinement = pose_refinement;
    flat_tags(&o, ntags, tags, listed_only);
    auto* h = new MultiShellHarness();
    h->node.reset(new amd::isaac_ros::apriltag::AprilTagMultiCameraNode(o, static_cast<uint32_t>(num_streams)));
    h->node->set_auto_flush(auto_flush != 0);
    h->last.resize(num_streams); h->last_tf.resize(num_streams); h->publishes.assign(num_streams, 0);
    h->node->set_detections_callback([h](uint32_t s, const AprilTagDetectionArray& m) { h->last[s] = m; h->publishes[s]++; });
    h->node->set_transforms_callback([h](uint32_t s, const std::vector<TransformStamped>& t) { h->last_tf[s] = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}
MultiShellHarness* node_shell_multi_create_refined(int num_streams, int max_tags, double size, int tile_size, const char* tag_family,
                                                   const char* backends, int decimate, int auto_flush, uint32_t pose_refinement,
                                                   char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    o.pose_refinement = pose_refinement;
    auto* h = new MultiShellHarness();
    h->node.reset(new amd::isaac_ros::apriltag::AprilTagMultiCameraNode(o, static_cast<uint32_t>(num_streams)));
    h->node->set_auto_flush(auto_flush != 0);
    h->last.resize(num_streams); h->last_tf.resize(num_streams); h->publishes.assign(num_streams, 0);
    h->node->set_detections_callback([h](uint32_t s, const AprilTagDetectionArray& m) { h->last[s] = m; h->publishes[s]++; });
    h->node->set_transforms_callback([h](uint32_t s, const std::vector<TransformStamped>& t) { h->last_tf[s] = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}
MultiShellHarness* node_shell_multi_create_covariance(int num_streams, int max_tags, double size, int tile_size, const char* tag_family,
                                                      const char* backends, int decimate, int auto_flush, uint32_t pose_refinement,
                                                      int nbundles, const NodeShellRigidBundle* bundles, double pose_covariance_sigma_px,
                                                      char* err, size_t err_len) {
  try {
    NodeOptions o;
    o.max_tags = max_tags; o.size = size; o.tile_size = static_cast<uint16_t>(tile_size);
    o.tag_family = tag_family; o.backends = backends; o.decimate = static_cast<uint32_t>(decimate);
    o.pose_refinement = pose_refinement;
    set_rigid_bundle_options(&o, nbundles, bundles);
    o.pose_covariance_sigma_px = pose_covariance_sigma_px;
    auto* h = new MultiShellHarness();
    h->node.reset(new amd::isaac_ros::apriltag::AprilTagMultiCameraNode(o, static_cast<uint32_t>(num_streams)));
    h->node->set_auto_flush(auto_flush != 0);
    h->last.resize(num_streams); h->last_tf.resize(num_streams); h->publishes.assign(num_streams, 0);
    h->node->set_detections_callback([h](uint32_t s, const AprilTagDetectionArray& m) { h->last[s] = m; h->publishes[s]++; });
    h->node->set_transforms_callback([h](uint32_t s, const std::vector<TransformStamped>& t) { h->last_tf[s] = t; });
    return h;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return nullptr;
  }
}
int node_shell_multi_last_covariances(MultiShellHarness* h, int stream, double* out36, int max_out) {
  return copy_covariances(h->last[stream], out36, max_out);
}
int node_shell_multi_last_rigid_covariances(MultiShellHarness* h, int stream, double* out36, int max_out) {
  return copy_rigid_covariances(h->node->last_rigid_bundle_poses(static_cast<uint32_t>(stream)), out36, max_out);
}
int node_shell_multi_last_transforms(MultiShellHarness* h, int stream, NodeShellTransform* out, int max_out) {
  return copy_transforms(h->last_tf[stream], out, max_out);
}
int node_shell_multi_last_bundle_poses(MultiShellHarness* h, int stream, NodeShellBundlePose* out, int max_out) {
  return copy_bundle_poses(h->node->last_bundle_poses(static_cast<uint32_t>(stream)), out, max_out);
}

void node_shell_multi_destroy(MultiShellHarness* h) { delete h; }

// 1 staged, 0 not (stamps differ / dropped), -2 exception
int node_shell_multi_on_frame_full(MultiShellHarness* h, int stream, const uint8_t* data, int is_device, const char* encoding,
                                   uint32_t width, uint32_t height, uint32_t step, const double* k9, const double* d, int nd,
                                   const char* distortion_model, const double* p12, const double* r9, const char* frame_id, int32_t sec,
                                   uint32_t nanosec, int32_t info_sec, uint32_t info_nanosec, char* err, size_t err_len) {
  try {
    Image img;
    img.header.frame_id = "image_frame"; img.header.stamp.sec = sec; img.header.stamp.nanosec = nanosec;
    img.width = width; img.height = height; img.step = step; img.encoding = encoding; img.data = data; img.is_device = is_device != 0;
    CameraInfo info;
    info.header.frame_id = frame_id; info.header.stamp.sec = info_sec; info.header.stamp.nanosec = info_nanosec;
    info.width = width; info.height = height;
    for (int i = 0; i < 9; i++) info.k[i] = k9[i];
    fill_camera_info_extras(&info, d, nd, distortion_model, p12, r9);
    return h->node->CameraImageCallback(static_cast<uint32_t>(stream), img, info) ? 1 : 0;
  } catch (const std::exception& e) {
    if (err && err_len) { std::strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return -2;
  }
}

int node_shell_multi_on_frame_info(MultiShellHarness* h, int stream, const uint8_t* data, int is_device, const char* encoding,
                                   uint32_t width, uint32_t height, uint32_t step, const double* k9, const double* d, int nd,
                                   const char* distortion_model, const double* p12, const char* frame_id, int32_t sec, uint32_t nanosec,
                                   int32_t info_sec, uint32_t info_nanosec, char* err, size_t err_len) {
  return node_shell_multi_on_frame_full(h, stream, data, is_device, encoding, width, height, step, k9, d, nd, distortion_model, p12,
                                        nullptr, frame_id, sec, nanosec, info_sec, info_nanosec, err, err_len);
}

int node_shell_multi_on_frame(MultiShellHarness* h, int stream, const uint8_t* data, int is_device, const char* encoding, uint32_t width,
                              uint32_t height, uint32_t step, const double* k9, const char* frame_id, int32_t sec, uint32_t nanosec,
                              int32_t info_sec, uint32_t info_nanosec, char* err, size_t err_len) {
  return node_shell_multi_on_frame_info(h, stream, data, is_device, encoding, width, height, step, k9, nullptr, 0, nullptr, nullptr,
                                        frame_id, sec, nanosec, info_sec, info_nanosec, err, err_len);
}

int node_shell_multi_flush(MultiShellHarness* h) { return static_cast<int>(h->node->Flush()); }
int node_shell_multi_publishes(MultiShellHarness* h, int stream) { return h->publishes[stream]; }

// the last message published for `stream`: number of detections (records in out), header frame / stamp through the outputs
int node_shell_multi_last(MultiShellHarness* h, int stream, NodeShellDetection* out, int max_out, char* out_frame_id, size_t frame_id_len,
                          int32_t* sec, uint32_t* nanosec) {
  const auto& m = h->last[stream];
  if (out_frame_id && frame_id_len) { std::strncpy(out_frame_id, m.header.frame_id.c_str(), frame_id_len - 1); out_frame_id[frame_id_len - 1] = 0; }
  if (sec) *sec = m.header.stamp.sec;
  if (nanosec) *nanosec = m.header.stamp.nanosec;
  const int n = static_cast<int>(m.detections.size());
  for (int i = 0; i < n && i < max_out; i++) {
    const auto& d = m.detections[i];
    NodeShellDetection& o = out[i];
    std::memset(&o, 0, sizeof(o));
    o.id = d.id;
    std::strncpy(o.family, d.family.c_str(), sizeof(o.family) - 1);
    o.center[0] = d.center.x; o.center[1] = d.center.y;
    for (int c = 0; c < 4; c++) { o.corners[c][0] = d.corners[c].x; o.corners[c][1] = d.corners[c].y; }
    o.position[0] = d.pose.pose.pose.position.x; o.position[1] = d.pose.pose.pose.position.y; o.position[2] = d.pose.pose.pose.position.z;
    o.orientation_xyzw[0] = d.pose.pose.pose.orientation.x; o.orientation_xyzw[1] = d.pose.pose.pose.orientation.y;
    o.orientation_xyzw[2] = d.pose.pose.pose.orientation.z; o.orientation_xyzw[3] = d.pose.pose.pose.orientation.w;
    std::strncpy(o.child_frame_id, h->last_tf[stream][i].child_frame_id.c_str(), sizeof(o.child_frame_id) - 1);
  }
  return n;
}

}  // extern "C"
