// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY (see ros/ros.h).  Plain struct of the message's field list
// (std_msgs/Header header, bool success, uint8 gait_cycles, uint8 gait_cycles_succeed, Foothold[] footholds).
#pragma once
#include <foothold_planner_msgs/Foothold.h>
namespace foothold_planner_msgs {
struct GlobalFootholds {
    std_msgs::Header header;
    uint8_t success = 0;
    uint8_t gait_cycles = 0;
    uint8_t gait_cycles_succeed = 0;
    std::vector<Foothold> footholds;
};
}  // namespace foothold_planner_msgs
