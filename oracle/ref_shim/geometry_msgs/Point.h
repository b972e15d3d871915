// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY (see ros/ros.h).  Plain structs; fields zero as ROS messages construct.
#pragma once
#include <ostream>
#include <vector>
#include <std_msgs/Header.h>
namespace geometry_msgs {
struct Point {
    double x = 0, y = 0, z = 0;
};
struct Vector3 {
    double x = 0, y = 0, z = 0;
};
struct Point32 {
    float x = 0, y = 0, z = 0;
};
struct Quaternion {
    double x = 0, y = 0, z = 0, w = 0;
};
struct Pose {
    Point position;
    Quaternion orientation;
};
struct Polygon {
    std::vector<Point32> points;
};
inline std::ostream& operator<<(std::ostream& os, const Point& p) {
    return os << "x: " << p.x << "\ny: " << p.y << "\nz: " << p.z << "\n";
}
inline std::ostream& operator<<(std::ostream& os, const Vector3& p) {
    return os << "x: " << p.x << "\ny: " << p.y << "\nz: " << p.z << "\n";
}
}  // namespace geometry_msgs
