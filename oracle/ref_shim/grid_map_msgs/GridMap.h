// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY (see ros/ros.h).  The reference only hands this message from the
// subscriber to GridMapRosConverter::fromMessage and from toMessage to a publisher; the fields are the shim's own:
// geometry plus one column-major f32 array per layer (start index 0).
#pragma once
#include <geometry_msgs/Point.h>
namespace grid_map_msgs {
struct GridMapInfo {
    std_msgs::Header header;
    double resolution = 0;
    double length_x = 0, length_y = 0;
    geometry_msgs::Pose pose;
};
struct GridMap {
    GridMapInfo info;
    int32_t rows = 0, cols = 0;
    std::vector<std::string> layers;
    std::vector<std::vector<float>> data;
};
}  // namespace grid_map_msgs
