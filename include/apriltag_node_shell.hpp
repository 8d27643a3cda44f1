// apriltag_node_shell.hpp -- ROS-free C++ mirror of the reference node surface
// nvidia::isaac_ros::apriltag::AprilTagNode
//   (reference include/isaac_ros_apriltag/apriltag_node.hpp:48-91, src/apriltag_node.cpp:562-633),
// with the message types reduced to plain structs that carry the same field names the node reads and
// writes (sensor_msgs/Image, sensor_msgs/CameraInfo, isaac_ros_apriltag_interfaces/AprilTagDetection
// [Array], geometry_msgs/TransformStamped; fields as used at src/apriltag_node.cpp:324-363,500-546).
//
// ROS 2 is not present in the build image, so this shell keeps the node's logic -- parameters and their
// defaults, backend/family validation and its error text, lazy initialisation on the first frame from
// CameraInfo (K, not P), encoding check, message assembly, TF naming, error policy -- behind callbacks
// instead of rclcpp publishers.  An rclcpp component is a thin adapter over this class.
#pragma once
#include <array>
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

namespace amd {
namespace isaac_ros {
namespace apriltag {

struct Time { int32_t sec = 0; uint32_t nanosec = 0; };
struct Header { Time stamp; std::string frame_id; };

// sensor_msgs/Image.  `data` may be host memory (is_device = false: copied to the GPU, as a plain
// sensor_msgs subscriber would) or a device pointer (is_device = true: the NITROS-handle case,
// src/apriltag_node.cpp:480-486).
struct Image {
  Header header;
  uint32_t height = 0, width = 0;
  std::string encoding;
  uint32_t step = 0;
  const uint8_t* data = nullptr;
  bool is_device = false;
  bool is_bigendian = false;   // sensor_msgs/Image.is_bigendian: read for the 16-bit encodings, whose big-endian frames are dropped
};

struct CameraInfo {
  Header header;
  uint32_t height = 0, width = 0;
  std::array<double, 9> k{};  // the node reads K (k[0],k[4],k[2],k[5]), src/apriltag_node.cpp:442-446
  // read only with NodeOptions::rectify (RectificationModel below) or rectify_full (RectificationModelEx)
  std::vector<double> d;            // distortion coefficients: k1, k2, p1, p2, k3 of "plumb_bob" (fewer: zero-padded)
  std::string distortion_model;     // "plumb_bob" or empty; with rectify_full also "rational_polynomial" and "equidistant"
  std::array<double, 12> p{};       // projection matrix: its left 3x3 is the rectified image's camera when p[0] != 0
  std::array<double, 9> r{};        // rectification rotation (rectify_full only); all zero, as a driver that never fills it leaves it: the identity
};

// The camera model NodeOptions::rectify hands the detector (amdAprilTagsCameraModel_t): K and D of the distorted image, and the
// pinhole camera Knew of the rectified one -- the left 3x3 of P when p[0] != 0, K otherwise.
struct CameraModel {
  std::array<double, 9> k{};
  std::array<double, 5> d{};
  std::array<double, 9> knew{};
};
// Throws std::runtime_error for a distortion_model other than "plumb_bob" / empty and for more than five coefficients.
CameraModel RectificationModel(const CameraInfo& camera_info);

// The camera model NodeOptions::rectify_full hands the detector (amdAprilTagsCameraModelEx_t): kind is amdAprilTagsDistortion --
// "plumb_bob" or empty 0, "rational_polynomial" 1, "equidistant" 2 -- with up to 5, 8 and 4 coefficients, zero-padded; r is
// CameraInfo::r, the identity where that is all zero; knew as in CameraModel.
struct CameraModelEx {
  uint32_t kind = 0;
  std::array<double, 9> k{};
  std::array<double, 8> d{};
  std::array<double, 9> r{};
  std::array<double, 9> knew{};
};
// Throws std::runtime_error for any other distortion_model (the text names the three known ones) and for more coefficients than
// the model has.
CameraModelEx RectificationModelEx(const CameraInfo& camera_info);

struct Point { double x = 0, y = 0, z = 0; };
struct Quaternion { double x = 0, y = 0, z = 0, w = 1; };
struct Pose { Point position; Quaternion orientation; };
struct PoseWithCovariance { Pose pose; std::array<double, 36> covariance{}; };
struct PoseWithCovarianceStamped { Header header; PoseWithCovariance pose; };

struct AprilTagDetection {
  std::string family;
  int32_t id = 0;
  Point center;
  std::array<Point, 4> corners;
  PoseWithCovarianceStamped pose;
};
struct AprilTagDetectionArray { Header header; std::vector<AprilTagDetection> detections; };

struct Vector3 { double x = 0, y = 0, z = 0; };
struct Transform { Vector3 translation; Quaternion rotation; };
struct TransformStamped { Header header; std::string child_frame_id; Transform transform; };

// A tag bundle (apriltag_ros' word): a planar board of tags of the node's family whose pose the detector solves per frame from all its
// detected tags at once (amdAprilTagsSetBundles, include/apriltag_amd.h).  (x, y): the tag centre on the board plane in metres, size:
// its black-border edge; tag axes parallel to the board axes.
struct BundleMember { uint32_t id = 0; double x = 0, y = 0, size = 0; };
struct Bundle {
  std::string name;                 // at most 31 characters: the TF child frame is "bundle:<name>"
  std::vector<BundleMember> members;
  uint32_t max_hamming = 2;         // a tag is used only with at most this many bit errors ...
  double min_decision_margin = 0;   // ... and at least this decision margin
  uint32_t min_tags = 1;            // with fewer used tags the bundle is not solved (no transform)
};
// The detector's record of one bundle for one frame (amdAprilTagsBundlePose_t): status 0 solved, 1 too few tags, 2 singular.
struct BundlePose {
  std::string name;
  uint32_t status = 0, ntags = 0, nskipped = 0;
  std::array<double, 9> R{};        // row-major
  std::array<double, 3> t{};
  double sq_err_sum = 0;            // squared pixel reprojection errors of the 4 * ntags corners, summed
};

// A rigid 3-D tag bundle (amdAprilTagsSetBundlesEx): a cube, a rig, a board with turned tags.  Every member carries its pose in the
// bundle frame as apriltag_ros' bundles do -- the tag centre (x, y, z) in metres and the orientation as a quaternion (qw, qx, qy, qz),
// which the shell divides by its norm before it forms the rotation -- and its black-border edge.
struct RigidBundleMember { uint32_t id = 0; double x = 0, y = 0, z = 0; double qw = 1, qx = 0, qy = 0, qz = 0; double size = 0; };
struct RigidBundle {
  std::string name;                 // at most 31 characters: the TF child frame is "bundle:<name>"
  std::vector<RigidBundleMember> members;   // at most 64
  uint32_t max_hamming = 2;
  double min_decision_margin = 0;
  uint32_t min_tags = 1;
  uint32_t iterations = 50;         // steps of each of the two chains
};
// The detector's record of one rigid bundle for one frame (amdAprilTagsBundlePoseEx_t): status 0 solved, 1 too few tags, 3 degenerate.
struct RigidBundlePose {
  std::string name;
  uint32_t status = 0, ntags = 0, nskipped = 0, seed = 0, chosen = 0;
  std::array<double, 9> R{}, R_alt{};   // row-major
  std::array<double, 3> t{}, t_alt{};
  double err = 0, sq_err_sum = 0, err_alt = 0, sq_err_sum_alt = 0;
  // NodeOptions::pose_covariance_sigma_px: the chosen pose's covariance as PoseWithCovariance's (zeros: off, or not valid)
  std::array<double, 36> covariance{};
};

// One camera of a calibrated rig (amdAprilTagsSetRig): the RIG frame in the CAMERA frame, X_cam = R X_rig + t, R row-major and a
// rotation as it stands (the library refuses max |R R^T - I| > 1e-6 or det R <= 0).
struct RigCamera {
  std::array<double, 9> R{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
  std::array<double, 3> t{};
};
// The detector's record of one rigid bundle for one round of a rig (amdAprilTagsRigBundlePose_t): the bundle frame in the rig frame
// from the tags of all the round's cameras.  seed_stream: the stream of the seed observation.
struct RigBundlePose {
  std::string name;
  uint32_t status = 0, nobs = 0, nskipped = 0, ndropped = 0, ncams = 0, seed_stream = 0, seed = 0, chosen = 0;
  std::array<double, 9> R{}, R_alt{};   // row-major
  std::array<double, 3> t{}, t_alt{};
  double err = 0, sq_err_sum = 0, err_alt = 0, sq_err_sum_alt = 0;
};

// One tag of a deployment (NodeOptions::tags; apriltag_ros: standalone_tags [{id, size, name}]; ROS 2 apriltag_ros: tag.ids /
// tag.sizes / tag.frames).
struct TagSpec {
  std::string family;   // empty: NodeOptions::tag_family (the node decodes that one family: another name is refused)
  uint32_t id = 0;
  double size = 0;      // the tag's edge in metres; 0: NodeOptions::size
  std::string frame;    // the TF child frame of the tag; empty: "family:id".  At most 47 characters.
};

// Parameters declared in the constructor of the reference node (src/apriltag_node.cpp:564-568).
struct NodeOptions {
  int max_tags = 64;
  double size = 0.22;
  uint16_t tile_size = 4;
  std::string tag_family = "tag36h11";
  std::string backends = "CUDA";  // reference default VPI_BACKEND_CUDA; "CUDA" | "HIP" | "GPU" select this library
  uint32_t decimate = 1;          // extension (AprilRobotics quad_decimate); 1 = cuAprilTags behaviour
  double quad_sigma = 0.0;        // extension (AprilRobotics quad_sigma, apriltag_ros `blur` / `sigma`): blur > 0, sharpen < 0, |.| <= 4;
                                  // applied with amdAprilTagsSetQuadSigma when the handle is created; 0 = cuAprilTags behaviour
  // The reference's cuAprilTags branch (backends == "CUDA") throws on every encoding but rgb8 / bgr8
  // (src/apriltag_node.cpp:469-476); its VPI branch takes the five of :76-82.  This shell takes the five in BOTH modes by default --
  // a superset: mono8 is what north_star feeds the detector, and the library's colour entry point reads rgba8 / bgra8 as well.
  // true: cuAprilTags mode refuses everything but rgb8 / bgr8 with the reference's own text.
  bool strict_cuapriltags_encodings = false;
  // Extension (AprilTagNode): beside the five, the node hands the raw formats of industrial cameras through as they arrive --
  // "bayer_rggb8", "bayer_bggr8", "bayer_gbrg8", "bayer_grbg8", "mono16", "bayer_rggb16", "bayer_bggr16", "bayer_gbrg16",
  // "bayer_grbg16" -- and the submission turns them into gray.  raw_shift: the sample of a 16-bit encoding is
  // min(255, s >> raw_shift), 0 .. 8 (amdAprilTagsSetRawShift; a sensor with 12 significant bits sets 4).  A 16-bit frame with
  // is_bigendian set is dropped; strict_cuapriltags_encodings refuses all nine as it refuses mono8.
  uint32_t raw_shift = 8;
  // AprilTagMultiCameraNode only (AprilTagNode, the single-camera shape of the reference, ignores them): the largest frame of a mixed
  // rig.  Both set: the handle is created at max_width x max_height with per-frame image sizes on (amdAprilTagsSetPerFrameSizes), and
  // streams of every admissible size are batched together.  0 (the default): one size, the first frame's; other sizes are dropped.
  uint32_t max_width = 0, max_height = 0;
  // Extension: the frames come from a distorted camera and are undistorted INSIDE the detector's submission (amdAprilTagsSetRectification;
  // the reference puts a RectifyNode in front, launch/isaac_ros_apriltag_usb_cam.launch.py:43-63).  The model is RectificationModel of the
  // stream's CameraInfo (AprilTagNode: of the first frame's, like K; AprilTagMultiCameraNode: of every staged frame's, set before each
  // flush in slot order), and the pose is computed with Knew -- fx, fy, cx, cy, and its [0][1] as the skew in VPI mode -- in place of K.
  bool rectify = false;
  // The same for every camera a CameraInfo describes (amdAprilTagsSetRectificationEx): the model is RectificationModelEx -- the three
  // distortion models, and the rectification rotation r of a stereo head.  Turns rectification on by itself; with it off `rectify`
  // takes plumb_bob alone and ignores r, as it always has.  The pose is reported in the rectified camera's frame.
  bool rectify_full = false;
  // Extension: raw-frame mode (amdAprilTagsSetCornerUndistortion), in place of `rectify` / `rectify_full` (both kinds set is an error):
  // the frames are detected as the camera delivers them and the corners of the detections are undistorted, not the pixels.  The model is
  // RectificationModelEx of the stream's CameraInfo, taken and set as `rectify_full` takes and sets it (with resize_width x resize_height
  // its K and Knew are scaled to the resized image, which is the one detected), and the pose is computed with Knew.  The detections'
  // corners and centre stay the raw frame's; their poses, the "family:id" transforms, the bundle transforms, the refined poses and the
  // covariances are those of the undistorted corners.  A detection whose corners cannot be undistorted (AMDAT_UNDISTORT_INVALID) is
  // published with a zero translation and the identity orientation -- with pose_refinement on as well: the refined record of such a
  // detection (AMDAT_POSE_DEGENERATE, all zero) is not taken.
  bool undistort_corners = false;
  // Extension: every frame is resized to resize_width x resize_height INSIDE the detector's submission, behind the rectification where
  // `rectify` is set (amdAprilTagsSetResize; the reference puts a ResizeNode in front and recommends it for 4K input, README.md:16-29).
  // Both set: AprilTagNode creates its handle at that size, AprilTagMultiCameraNode at that size too (or at max_width x max_height with
  // per-frame image sizes where those are set); frames of ANY size (1 .. 16384 a side) are accepted instead of dropped; the resize is set
  // once; and the pose is computed with the camera of the resized image, image_proc's convention: fx, cx and the skew of K (`rectify`:
  // of Knew) times resize_width / width, fy and cy times resize_height / height -- of the first frame's CameraInfo for AprilTagNode,
  // of every staged frame's for AprilTagMultiCameraNode.  0 (the default): off.
  uint32_t resize_width = 0, resize_height = 0;
  // Extension: tag bundles, set once when the handle is created (amdAprilTagsSetBundles).  Both nodes append one TransformStamped per
  // SOLVED bundle behind the tags' -- child frame "bundle:<name>", the camera info's header, as for tags -- and keep the frame's records
  // (last_bundle_poses).  Empty (the default): off.
  std::vector<Bundle> bundles;
  // Extension: rigid 3-D tag bundles, set once when the handle is created (amdAprilTagsSetBundlesEx), in place of `bundles` (one kind
  // at a time: both set is an error).  Both nodes append one TransformStamped per SOLVED bundle behind the tags', from the chosen
  // pose -- child frame "bundle:<name>" -- and keep the frame's records (last_rigid_bundle_poses).  Empty (the default): off.
  std::vector<RigidBundle> rigid_bundles;
  // Extension: the orthogonal-iteration tag pose with both minima (amdAprilTagsSetPoseRefinement), set once when the handle is
  // created: this many iterations per chain, 50 being AprilRobotics' estimate_tag_pose.  With it on, the pose of every detection and
  // its "family:id" transform are the chosen refined pose in place of the homography pose.  0 (the default): off.
  uint32_t pose_refinement = 0;
  // Extension: pose covariance (amdAprilTagsSetPoseCovariance), set once when the handle is created: the standard deviation, in
  // pixels, of the independent error the caller ascribes to every corner coordinate.  With it on and pose_refinement > 0, both nodes
  // fill detection.pose.pose.covariance with the chosen pose's 36 doubles -- row-major in ROS' order (x, y, z, rotation about x, y,
  // z; camera optical frame), copied without conversion -- and every RigidBundlePose carries its `covariance` the same way.  A record
  // whose covariance is not valid keeps zeros.  0 (the default): off, the covariance all zero as the reference node leaves it.
  double pose_covariance_sigma_px = 0;
  // Extension, AprilTagMultiCameraNode only (AprilTagNode ignores both): the streams are the cameras of one calibrated rig
  // (amdAprilTagsSetRig, set once when the handle is created), rig_cameras[s] being stream s's extrinsics -- one per stream, with
  // rigid_bundles set.  Every Flush is one instant: it sends a slot map with every served stream in group 0 as its own camera (a
  // stream without a staged frame is simply absent), and, behind the per-stream transforms, one TransformStamped per SOLVED bundle
  // from the rig record's chosen pose -- child frame "rig_bundle:<name>", parent rig_frame_id, the stamp of the round's first served
  // stream, handed to the transforms callback with that stream's -- and keeps the round's records (last_rig_bundle_poses).  Empty
  // (the default): off.
  std::vector<RigCamera> rig_cameras;
  std::string rig_frame_id = "rig";
  // Extension: the tag table (amdAprilTagsSetTagTable), set once when the handle is created.  Every listed tag's pose -- the homography
  // pose, and with the other extensions its twin's, its refined pose and its covariance -- is that of a tag of its own size, and its
  // transform's child frame is its `frame` where that is not empty; a tag without an entry keeps NodeOptions::size and "family:id".
  // The message's family and id fields do not change.  tags_listed_only: a tag without an entry is not reported at all -- no
  // detection, no transform, no place among max_tags (members of `bundles` / `rigid_bundles` included: list them).  Refused when
  // the node is constructed: a family other than tag_family, a frame above 47 characters, two entries for one id, a negative or
  // non-finite size, more than 4096 entries; an id beyond the family's codes is refused when the handle is created.  Empty (the
  // default): off.
  std::vector<TagSpec> tags;
  bool tags_listed_only = false;
};

class AprilTagNode {
 public:
  using DetectionsCallback = std::function<void(const AprilTagDetectionArray&)>;
  using TransformsCallback = std::function<void(const std::vector<TransformStamped>&)>;

  // Throws std::runtime_error whose what() contains
  // "Tag family not supported by specified backend" (src/apriltag_node.cpp:584-599).
  explicit AprilTagNode(const NodeOptions& options);
  ~AprilTagNode();

  // "tag_detections" publisher / TF broadcaster stand-ins (src/apriltag_node.cpp:548-549).
  void set_detections_callback(DetectionsCallback cb);
  void set_transforms_callback(TransformsCallback cb);

  // Synchronised image + camera_info (ExactTime policy upstream, include/.../apriltag_node.hpp:74-78):
  // returns false (and does nothing) unless both stamps are identical.
  bool CameraImageCallback(const Image& image, const CameraInfo& camera_info);

  const NodeOptions& options() const;
  bool initialized() const;
  // NodeOptions::bundles: the records of the last published frame, one per bundle in the options' order (empty: bundles off)
  const std::vector<BundlePose>& last_bundle_poses() const;
  // NodeOptions::rigid_bundles: the same for the rigid kind
  const std::vector<RigidBundlePose>& last_rigid_bundle_poses() const;

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

// Batching front end: S camera streams on ONE GPU, one detector submission per round -- streams of one image size, or (NodeOptions::
// max_width / max_height) of any size up to that one.
//
// The reference node -- and AprilTagNode above -- hands the detector one frame per call (src/apriltag_node.cpp:491-493);
// S cameras then mean S nodes and S one-frame submissions, each a chain of ~20 dependent kernels that leaves the GPU
// mostly idle (1 200 frames/s per call stream against ~10 000 batched).  This node keeps the reference's
// per-stream surface -- parameters, ExactTime pairing, the five encodings, lazy initialisation from the first
// CameraInfo, message assembly with the stream's own camera_info header, TF child "<family>:<id>" under the stream's
// camera frame (src/apriltag_node.cpp:499-549) -- but stages the latest frame of every stream on the device and submits
// all staged frames as ONE amdAprilTagsDetectBatch with per-frame intrinsics (each stream's own K).  Results are
// bit-identical to S independent AprilTagNode instances (tests/test_gpu_parity.py::test_multi_camera_node).
class AprilTagMultiCameraNode {
 public:
  using DetectionsCallback = std::function<void(uint32_t stream, const AprilTagDetectionArray&)>;
  using TransformsCallback = std::function<void(uint32_t stream, const std::vector<TransformStamped>&)>;

  // Same validation and error text as AprilTagNode.  All streams share the options (family, tag size, backends).
  AprilTagMultiCameraNode(const NodeOptions& options, uint32_t num_streams);
  ~AprilTagMultiCameraNode();
  void set_detections_callback(DetectionsCallback cb);
  void set_transforms_callback(TransformsCallback cb);

  // Stages one synchronised pair of `stream` (a newer pair replaces an unsubmitted older one: "latest frame").  Returns
  // false when the stamps differ (ExactTime would not fire) or the frame is dropped (size mismatch, as AprilTagNode; with max_width /
  // max_height set: a frame larger than that, or too small for one threshold tile).
  // With auto_flush (default) the round is submitted as soon as every stream has a staged frame.
  bool CameraImageCallback(uint32_t stream, const Image& image, const CameraInfo& camera_info);
  // Submits the staged frames of all streams that have one; publishes per stream; returns the number of streams served.
  uint32_t Flush();
  void set_auto_flush(bool on);

  uint32_t num_streams() const;
  const NodeOptions& options() const;
  // NodeOptions::bundles: the records of the last frame published for `stream`, one per bundle in the options' order
  const std::vector<BundlePose>& last_bundle_poses(uint32_t stream) const;
  const std::vector<RigidBundlePose>& last_rigid_bundle_poses(uint32_t stream) const;
  // NodeOptions::rig_cameras: the rig records of the last round, one per rigid bundle in the options' order (empty: the rig is off)
  const std::vector<RigBundlePose>& last_rig_bundle_poses() const;

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

}  // namespace apriltag
}  // namespace isaac_ros
}  // namespace amd
