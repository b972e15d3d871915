// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY (see ros/ros.h).
#pragma once
#include <geometry_msgs/Point.h>
namespace geometry_msgs {
struct PointStamped {
    std_msgs::Header header;
    Point point;
};
}  // namespace geometry_msgs
