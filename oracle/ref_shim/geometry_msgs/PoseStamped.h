// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY (see ros/ros.h).
#pragma once
#include <geometry_msgs/Point.h>
namespace geometry_msgs {
struct PoseStamped {
    std_msgs::Header header;
    Pose pose;
};
}  // namespace geometry_msgs
