// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY (see ros/ros.h).
#pragma once
#include <geometry_msgs/Point.h>
namespace geometry_msgs {
struct PolygonStamped {
    std_msgs::Header header;
    Polygon polygon;
};
}  // namespace geometry_msgs
