// apriltag_node_component.cpp -- rclcpp component with the reference's plugin identity
// (class nvidia::isaac_ros::apriltag::AprilTagNode, node name "apriltag_node", topics image / camera_info
// in, tag_detections + /tf out; reference src/apriltag_node.cpp:562-633, launch/isaac_ros_apriltag.launch.py:24-41)
// as a thin adapter over the ROS-free shell amd::isaac_ros::apriltag::AprilTagNode
// (include/apriltag_node_shell.hpp), which owns all of the node logic and talks to libapriltag_amd.so.
//
// NOT BUILT IN THIS REPOSITORY'S IMAGE: ROS 2 (rclcpp, message_filters, tf2_ros,
// isaac_ros_apriltag_interfaces) is absent there, so this file is compiled only by the colcon build
// described in ros2/README.md.  It takes sensor_msgs/Image (host memory); the NITROS zero-copy type
// adaptation of the reference is NVIDIA-proprietary and out of scope.
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "apriltag_node_shell.hpp"
#include "isaac_ros_apriltag_interfaces/msg/april_tag_detection_array.hpp"
#include "message_filters/subscriber.h"
#include "message_filters/sync_policies/exact_time.h"
#include "message_filters/synchronizer.h"
#include "rclcpp/rclcpp.hpp"
#include "sensor_msgs/msg/camera_info.hpp"
#include "sensor_msgs/msg/image.hpp"
#include "tf2_ros/transform_broadcaster.h"

namespace nvidia
{
namespace isaac_ros
{
namespace apriltag
{

namespace shell = amd::isaac_ros::apriltag;

class AprilTagNode : public rclcpp::Node
{
public:
  explicit AprilTagNode(const rclcpp::NodeOptions & options)
  : rclcpp::Node("apriltag_node", options),
    camera_image_sync_{ExactPolicy{3}, image_sub_, camera_info_sub_},
    detections_pub_{create_publisher<isaac_ros_apriltag_interfaces::msg::AprilTagDetectionArray>(
        "tag_detections", rclcpp::QoS(1))}
  {
    shell::NodeOptions opt;
    opt.max_tags = declare_parameter<int>("max_tags", 64);
    opt.size = declare_parameter<double>("size", 0.22);
    opt.tile_size = declare_parameter<uint16_t>("tile_size", 4);
    opt.tag_family = declare_parameter<std::string>("tag_family", "tag36h11");
    opt.backends = declare_parameter<std::string>("backends", "CUDA");  // name or comma list; exactly "CUDA" = cuAprilTags mode
    opt.decimate = static_cast<uint32_t>(declare_parameter<int>("decimate", 1));
    opt.quad_sigma = declare_parameter<double>("quad_sigma", 0.0);   // AprilRobotics quad_sigma (apriltag_ros `blur` / `sigma`)
    // Bayer and 16-bit image topics ("bayer_rggb8" .. "bayer_grbg16", "mono16") are taken as they arrive and turned into gray inside the
    // detector's submission, in place of an image_proc debayer node in front of this one.  raw_shift: the sample of a 16-bit encoding is
    // min(255, s >> raw_shift), 0 .. 8; a sensor with 12 significant bits sets 4
    opt.raw_shift = static_cast<uint32_t>(declare_parameter<int>("raw_shift", 8));
    // the image topic is the camera's distorted image: undistorted inside the detector's submission with camera_info's plumb_bob model
    // (K, D; the rectified camera is the left 3x3 of P), in place of a RectifyNode in front of this one
    opt.rectify = declare_parameter<bool>("rectify", false);
    // the same for every camera camera_info describes: plumb_bob, rational_polynomial or equidistant, behind its rectification
    // rotation R (either half of a stereo pair)
    opt.rectify_full = declare_parameter<bool>("rectify_full", false);
    // raw-frame mode, in place of both: the distorted image is detected as it stands and the detections' corners are undistorted under
    // that model; poses, transforms and covariances are those of the undistorted corners, in the rectified camera's frame
    opt.undistort_corners = declare_parameter<bool>("undistort_corners", false);
    // both set: every frame, whatever its size, is resized to resize_width x resize_height inside the detector's submission (behind the
    // rectification), in place of a ResizeNode in front of this one; the pose uses the camera scaled to that size.  0: off
    opt.resize_width = static_cast<uint32_t>(declare_parameter<int>("resize_width", 0));
    opt.resize_height = static_cast<uint32_t>(declare_parameter<int>("resize_height", 0));
    // tag bundles (planar boards solved per frame inside the detector's submission): bundle_names lists them, bundle_members holds five
    // numbers per member -- index into bundle_names, tag id, x, y of the tag centre on the board plane and its size, in metres.  One
    // "bundle:<name>" transform is broadcast per solved bundle.  Empty: off
    {
      const std::vector<std::string> names = declare_parameter<std::vector<std::string>>("bundle_names", std::vector<std::string>());
      const std::vector<double> members = declare_parameter<std::vector<double>>("bundle_members", std::vector<double>());
      for (const auto & n : names) {
        shell::Bundle b;
        b.name = n;
        opt.bundles.push_back(b);
      }
      for (size_t i = 0; i + 4 < members.size(); i += 5) {
        const size_t which = static_cast<size_t>(members[i]);
        if (which < opt.bundles.size()) {
          opt.bundles[which].members.push_back({static_cast<uint32_t>(members[i + 1]), members[i + 2], members[i + 3], members[i + 4]});
        }
      }
    }
    // rigid 3-D tag bundles (cubes, rigs, boards with turned tags, solved per frame as one rigid body): rigid_bundle_names lists them,
    // rigid_bundle_members holds ten numbers per member -- index into rigid_bundle_names, tag id, x, y, z of the tag centre in the
    // bundle frame in metres, its orientation qw, qx, qy, qz, and its size.  One "bundle:<name>" transform is broadcast per solved
    // bundle.  In place of bundle_names / bundle_members: one kind at a time.  Empty: off
    {
      const std::vector<std::string> names = declare_parameter<std::vector<std::string>>("rigid_bundle_names", std::vector<std::string>());
      const std::vector<double> members = declare_parameter<std::vector<double>>("rigid_bundle_members", std::vector<double>());
      for (const auto & n : names) {
        shell::RigidBundle b;
        b.name = n;
        opt.rigid_bundles.push_back(b);
      }
      for (size_t i = 0; i + 9 < members.size(); i += 10) {
        const size_t which = static_cast<size_t>(members[i]);
        if (which < opt.rigid_bundles.size()) {
          opt.rigid_bundles[which].members.push_back({static_cast<uint32_t>(members[i + 1]), members[i + 2], members[i + 3], members[i + 4],
                                                      members[i + 5], members[i + 6], members[i + 7], members[i + 8], members[i + 9]});
        }
      }
    }
    // the orthogonal-iteration tag pose with both minima (AprilRobotics' estimate_tag_pose) inside the detector's submission: this many
    // iterations per chain (50 upstream); the published poses and transforms are then the chosen refined pose.  0: off
    opt.pose_refinement = static_cast<uint32_t>(declare_parameter<int>("pose_refinement_iterations", 0));
    // pose covariance: the standard deviation, in pixels, of the independent error the caller ascribes to every corner coordinate.  With
    // pose_refinement_iterations > 0 the published pose.pose.covariance is then the first-order covariance of the chosen pose (x, y, z,
    // rotation about x, y, z in the camera optical frame), zeros where it could not be formed.  0: off, covariance all zero
    opt.pose_covariance_sigma_px = declare_parameter<double>("pose_covariance_sigma_px", 0.0);
    // camera rigs (one pose per instant and rigid bundle from the tags of all cameras of a calibrated rig): rig_cameras holds twelve
    // numbers per camera -- R row-major, then t, the rig frame in the camera frame, X_cam = R X_rig + t -- and rig_frame_id names the
    // parent frame of the "rig_bundle:<name>" transforms.  They are the batching front end's (shell::AprilTagMultiCameraNode, one
    // camera per stream); this single-camera component carries them in its options and ignores them, as the shell's AprilTagNode does
    {
      const std::vector<double> cams = declare_parameter<std::vector<double>>("rig_cameras", std::vector<double>());
      for (size_t i = 0; i + 11 < cams.size(); i += 12) {
        shell::RigCamera c;
        for (size_t k = 0; k < 9; k++) {c.R[k] = cams[i + k];}
        for (size_t k = 0; k < 3; k++) {c.t[k] = cams[i + 9 + k];}
        opt.rig_cameras.push_back(c);
      }
      opt.rig_frame_id = declare_parameter<std::string>("rig_frame_id", "rig");
    }
    // the tag table (the ROS 2 apriltag_ros' tag.ids / tag.frames / tag.sizes): tag_ids[i] has the edge tag_sizes[i] in metres (0: `size`)
    // and is published under the TF child frame tag_frames[i] (empty: "family:id"); the three lists have equal lengths.
    // tag_listed_only: tags that tag_ids does not name are not published at all
    {
      const std::vector<int64_t> ids = declare_parameter<std::vector<int64_t>>("tag_ids", std::vector<int64_t>());
      const std::vector<std::string> frames = declare_parameter<std::vector<std::string>>("tag_frames", std::vector<std::string>());
      const std::vector<double> sizes = declare_parameter<std::vector<double>>("tag_sizes", std::vector<double>());
      if (frames.size() != ids.size() || sizes.size() != ids.size()) {
        throw std::runtime_error("'tag_ids', 'tag_frames' and 'tag_sizes' must have equal lengths");
      }
      for (size_t i = 0; i < ids.size(); i++) {
        if (ids[i] < 0 || ids[i] > 65534) {throw std::runtime_error("'tag_ids': " + std::to_string(ids[i]) + " is no tag id");}
        shell::TagSpec t;
        t.id = static_cast<uint32_t>(ids[i]);
        t.size = sizes[i];
        t.frame = frames[i];
        opt.tags.push_back(t);
      }
      opt.tags_listed_only = declare_parameter<bool>("tag_listed_only", false);
    }
    // throws std::runtime_error("Tag family not supported by specified backend ...") like the reference
    impl_ = std::make_unique<shell::AprilTagNode>(opt);
    tf_broadcaster_ = std::make_unique<tf2_ros::TransformBroadcaster>(this);

    impl_->set_detections_callback(
      [this](const shell::AprilTagDetectionArray & in) {
        isaac_ros_apriltag_interfaces::msg::AprilTagDetectionArray msg;
        msg.header = last_info_header_;
        for (const auto & d : in.detections) {
          isaac_ros_apriltag_interfaces::msg::AprilTagDetection m;
          m.family = d.family;
          m.id = d.id;
          m.center.x = d.center.x;
          m.center.y = d.center.y;
          for (int i = 0; i < 4; i++) {
            m.corners.data()[i].x = d.corners[i].x;
            m.corners.data()[i].y = d.corners[i].y;
          }
          m.pose.pose.pose.position.x = d.pose.pose.pose.position.x;
          m.pose.pose.pose.position.y = d.pose.pose.pose.position.y;
          m.pose.pose.pose.position.z = d.pose.pose.pose.position.z;
          m.pose.pose.pose.orientation.x = d.pose.pose.pose.orientation.x;
          m.pose.pose.pose.orientation.y = d.pose.pose.pose.orientation.y;
          m.pose.pose.pose.orientation.z = d.pose.pose.pose.orientation.z;
          m.pose.pose.pose.orientation.w = d.pose.pose.pose.orientation.w;
          for (size_t i = 0; i < 36; i++) {m.pose.pose.covariance[i] = d.pose.pose.covariance[i];}
          msg.detections.push_back(m);
        }
        detections_pub_->publish(msg);
      });
    impl_->set_transforms_callback(
      [this](const std::vector<shell::TransformStamped> & in) {
        std::vector<geometry_msgs::msg::TransformStamped> tfs;
        for (const auto & t : in) {
          geometry_msgs::msg::TransformStamped tf;
          tf.header = last_info_header_;
          tf.child_frame_id = t.child_frame_id;
          tf.transform.translation.x = t.transform.translation.x;
          tf.transform.translation.y = t.transform.translation.y;
          tf.transform.translation.z = t.transform.translation.z;
          tf.transform.rotation.x = t.transform.rotation.x;
          tf.transform.rotation.y = t.transform.rotation.y;
          tf.transform.rotation.z = t.transform.rotation.z;
          tf.transform.rotation.w = t.transform.rotation.w;
          tfs.push_back(tf);
        }
        tf_broadcaster_->sendTransform(tfs);
      });

    camera_image_sync_.registerCallback(
      std::bind(&AprilTagNode::CameraImageCallback, this, std::placeholders::_1, std::placeholders::_2));
    image_sub_.subscribe(this, "image");
    camera_info_sub_.subscribe(this, "camera_info");
  }

private:
  void CameraImageCallback(
    const sensor_msgs::msg::Image::ConstSharedPtr & image,
    const sensor_msgs::msg::CameraInfo::ConstSharedPtr & camera_info)
  {
    shell::Image img;
    img.header.frame_id = image->header.frame_id;
    img.header.stamp.sec = image->header.stamp.sec;
    img.header.stamp.nanosec = image->header.stamp.nanosec;
    img.width = image->width;
    img.height = image->height;
    img.encoding = image->encoding;
    img.step = image->step;
    img.data = image->data.data();
    img.is_device = false;
    img.is_bigendian = image->is_bigendian != 0;
    shell::CameraInfo info;
    info.header.frame_id = camera_info->header.frame_id;
    info.header.stamp.sec = camera_info->header.stamp.sec;
    info.header.stamp.nanosec = camera_info->header.stamp.nanosec;
    info.width = camera_info->width;
    info.height = camera_info->height;
    for (int i = 0; i < 9; i++) {info.k[i] = camera_info->k[i];}
    info.d = camera_info->d;
    info.distortion_model = camera_info->distortion_model;
    for (int i = 0; i < 9; i++) {info.r[i] = camera_info->r[i];}
    for (int i = 0; i < 12; i++) {info.p[i] = camera_info->p[i];}
    last_info_header_ = camera_info->header;  // output headers = camera_info header (reference :501,:534)
    impl_->CameraImageCallback(img, info);
  }

  using ExactPolicy = message_filters::sync_policies::ExactTime<sensor_msgs::msg::Image, sensor_msgs::msg::CameraInfo>;
  message_filters::Subscriber<sensor_msgs::msg::Image> image_sub_;
  message_filters::Subscriber<sensor_msgs::msg::CameraInfo> camera_info_sub_;
  message_filters::Synchronizer<ExactPolicy> camera_image_sync_;
  rclcpp::Publisher<isaac_ros_apriltag_interfaces::msg::AprilTagDetectionArray>::SharedPtr detections_pub_;
  std::unique_ptr<tf2_ros::TransformBroadcaster> tf_broadcaster_;
  std::unique_ptr<shell::AprilTagNode> impl_;
  std_msgs::msg::Header last_info_header_;
};

}  // namespace apriltag
}  // namespace isaac_ros
}  // namespace nvidia

#include "rclcpp_components/register_node_macro.hpp"
RCLCPP_COMPONENTS_REGISTER_NODE(nvidia::isaac_ros::apriltag::AprilTagNode)
