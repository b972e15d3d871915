// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY (see grid_map_core/GridMap.hpp).
#pragma once
#include <geometry_msgs/PolygonStamped.h>
#include <grid_map_core/GridMap.hpp>
#include <grid_map_msgs/GridMap.h>

namespace grid_map {

class GridMapRosConverter {
public:
    static bool fromMessage(const grid_map_msgs::GridMap& m, GridMap& map) {
        fpo::GridMap g;
        g.setGeometry({m.info.length_x, m.info.length_y}, m.info.resolution, {m.info.pose.position.x, m.info.pose.position.y});
        if (g.size.i != m.rows || g.size.j != m.cols) return false;
        for (size_t k = 0; k < m.layers.size(); ++k) {
            if (m.data[k].size() != (size_t)m.rows * m.cols) return false;
            if (m.layers[k] == "traversability") g.trav = m.data[k];
            if (m.layers[k] == "elevation") g.elev = m.data[k];
        }
        map = GridMap(g, m.info.header.frame_id);
        return true;
    }
    static void toMessage(const GridMap& map, grid_map_msgs::GridMap& m) {
        const fpo::GridMap& g = map.geometry();
        m = grid_map_msgs::GridMap();
        m.info.header.frame_id = map.getFrameId();
        m.info.resolution = g.res;
        m.info.length_x = g.length.x;
        m.info.length_y = g.length.y;
        m.info.pose.position.x = g.position.x;
        m.info.pose.position.y = g.position.y;
        m.rows = g.size.i;
        m.cols = g.size.j;
        m.layers = map.getLayers();
        m.data.push_back(g.trav);
        if (!g.elev.empty()) m.data.push_back(g.elev);
    }
};

class PolygonRosConverter {
public:
    static void toMessage(const Polygon& polygon, geometry_msgs::PolygonStamped& m) {
        m.header.frame_id = polygon.getFrameId();
        m.polygon.points.clear();
        for (const fpo::Vec2& v : polygon.vertices()) {
            geometry_msgs::Point32 p;
            p.x = (float)v.x;
            p.y = (float)v.y;
            m.polygon.points.push_back(p);
        }
    }
};

}  // namespace grid_map
