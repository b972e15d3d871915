// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY (see grid_map_core/GridMap.hpp).
#pragma once
#include <grid_map_ros/GridMapRosConverter.hpp>
