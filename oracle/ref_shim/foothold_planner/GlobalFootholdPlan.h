// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY (see ros/ros.h).  Plain struct of the service's field lists
// (request: four geometry_msgs/Point current footholds and uint8 gait_cycles; response: GlobalFootholds footholds).
#pragma once
#include <foothold_planner_msgs/GlobalFootholds.h>
namespace foothold_planner {
struct GlobalFootholdPlan {
    struct Request {
        geometry_msgs::Point FR_current_foothold, RR_current_foothold, RL_current_foothold, FL_current_foothold;
        uint8_t gait_cycles = 0;
    };
    struct Response {
        foothold_planner_msgs::GlobalFootholds footholds;
    };
    Request request;
    Response response;
};
}  // namespace foothold_planner
