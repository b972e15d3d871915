// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY (see ros/ros.h).  The fields and constants the reference sets.
#pragma once
#include <geometry_msgs/Point.h>
namespace visualization_msgs {
struct Marker {
    enum : int32_t { ARROW = 0, CUBE = 1, SPHERE = 2, CYLINDER = 3, LINE_STRIP = 4, LINE_LIST = 5, CUBE_LIST = 6,
                     SPHERE_LIST = 7, POINTS = 8 };
    enum : int32_t { ADD = 0, MODIFY = 0, DELETE = 2 };
    std_msgs::Header header;
    std::string ns;
    int32_t id = 0;
    int32_t type = 0;
    int32_t action = 0;
    geometry_msgs::Pose pose;
    geometry_msgs::Vector3 scale;
    std_msgs::ColorRGBA color;
    ros::Duration lifetime;
    std::vector<geometry_msgs::Point> points;
};
}  // namespace visualization_msgs
