// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY (see ros/ros.h).  Plain struct of the message's field list
// (geometry_msgs/Point point, uint8 foot_id, uint8 gait_cycle_id).
#pragma once
#include <geometry_msgs/Point.h>
namespace foothold_planner_msgs {
struct Foothold {
    geometry_msgs::Point point;
    uint8_t foot_id = 0;
    uint8_t gait_cycle_id = 0;
};
}  // namespace foothold_planner_msgs
