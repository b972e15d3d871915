// REFERENCE DRIVER — TEST INFRASTRUCTURE ONLY.  Runs the REFERENCE's own FootholdPlanner (compiled in place from the
// reference tree against oracle/ref_shim/, see the Makefile) on one case file and writes what it computed as a flat
// array of doubles.  tests/golden/make_ref_golden.py writes the case files and parses the results.
//
//   ref_driver CASE OUT
//
// Case file (little endian): "FPREFC1\0", i32 mode (0 legs, 1 service), i32 rows, cols, f64 resolution, position x, y,
// f32 traversability[rows*cols] and elevation[rows*cols] (row-major), i32 nParams x {i32 len, key, i32 kind, f64 value |
// i32 len, string}, then
//   legs:    i32 n x {i32 kind (0 checkFoothold, 1 checkFootholdUseCentroidMethod, 2 getFootholdMeanHeight), f64 cx, cy,
//            f32 footRadius, f32 searchRadius, f64 vx[4], vy[4]}
//   service: i32 n x {f64 x, y, z, i32 gaitCycles}: one FRESH planner object per start pose; the pose reaches the
//            reference the only way it takes one — the initial_position/{x,y,z} parameters (initialize(), cpp:366-378).
// The reference prints heavily on stdout: it is pointed at /dev/null.  Its log files go to /home/<user>/laika_ws/log
// (cpp:3105; <user> from getpwuid, not $HOME, and dereferenced unchecked): this program answers getpwuid itself with a
// user whose home does not exist, so the opens fail silently, nothing is written anywhere and a uid without a passwd
// entry is no crash.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include "foothold_planner/FootholdPlanner.hpp"
#include <nlopt.hpp>

// file-scope state of the reference's translation unit (cpp:36, 50-51)
extern double lfCurrentRow, rhCurrentRow;
extern std::vector<int> nominalIndex, centroidIndex;
// ... and its tunable file-scope constants (cpp:34, 47-48): parameters "global/<name>" of a case set them
extern double ctol, hip_lower_scale, hip_upper_scale, skew_lower_scale, skew_upper_scale;

extern "C" struct passwd* getpwuid(uid_t) {
    static char name[] = "ref_driver_no_such_user";
    static struct passwd pw;
    pw.pw_name = name;
    return &pw;
}

namespace {

struct Reader {
    std::vector<char> buf;
    size_t at = 0;
    template <class T>
    T get() {
        T v;
        if (at + sizeof(T) > buf.size()) throw std::runtime_error("case file truncated");
        std::memcpy(&v, buf.data() + at, sizeof(T));
        at += sizeof(T);
        return v;
    }
    std::string str() {
        const int n = get<int32_t>();
        if (n < 0 || at + (size_t)n > buf.size()) throw std::runtime_error("case file truncated");
        std::string s(buf.data() + at, (size_t)n);
        at += (size_t)n;
        return s;
    }
};

struct Param {
    std::string key, text;
    int kind;
    double value;
};

struct Snapshot {  // the reference's globals as its objective sees them in one optimize() call
    int nominal[8], centroid[8];
    double lf, rh;
};

const double kNaN = std::numeric_limits<double>::quiet_NaN();

double g_lf0 = 0.0, g_rh0 = 0.0;  // lfCurrentRow / rhCurrentRow at the entry of a service call ("node start": 0)

void fillNode(ros::NodeHandle& nh, const std::vector<Param>& params) {
    for (const Param& p : params) {
        if (p.key == "global/ctol") ctol = p.value;
        else if (p.key == "global/hip_lower_scale") hip_lower_scale = p.value;
        else if (p.key == "global/hip_upper_scale") hip_upper_scale = p.value;
        else if (p.key == "global/skew_lower_scale") skew_lower_scale = p.value;
        else if (p.key == "global/skew_upper_scale") skew_upper_scale = p.value;
        else if (p.key == "global/lfCurrentRow") g_lf0 = p.value;
        else if (p.key == "global/rhCurrentRow") g_rh0 = p.value;
        else if (p.kind == 1)
            nh.setParam(p.key, p.text);
        else
            nh.setParam(p.key, p.value);
    }
}

void pushTrack(std::vector<double>& out, const ros::NodeHandle& nh, const char* topic) {
    const auto msgs = nh.published<foothold_planner_msgs::GlobalFootholds>(topic);
    out.push_back((double)msgs.size());
    if (msgs.empty()) return;
    const foothold_planner_msgs::GlobalFootholds& m = msgs.back();
    out.push_back(m.success);
    out.push_back(m.gait_cycles);
    out.push_back(m.gait_cycles_succeed);
    out.push_back((double)m.footholds.size());
    for (const auto& f : m.footholds) {
        out.push_back(f.foot_id);
        out.push_back(f.gait_cycle_id);
        out.push_back(f.point.x);
        out.push_back(f.point.y);
        out.push_back(f.point.z);
    }
}

void pushPath(std::vector<double>& out, const ros::NodeHandle& nh, const char* topic) {
    const auto msgs = nh.published<nav_msgs::Path>(topic);
    out.push_back((double)msgs.size());
    if (msgs.empty()) return;
    out.push_back((double)msgs.back().poses.size());
    for (const auto& p : msgs.back().poses) {
        out.push_back(p.pose.position.x);
        out.push_back(p.pose.position.y);
        out.push_back(p.pose.position.z);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: ref_driver CASE OUT\n");
        return 2;
    }
    Reader r;
    {
        std::ifstream f(argv[1], std::ios::binary);
        if (!f) {
            std::fprintf(stderr, "ref_driver: cannot read %s\n", argv[1]);
            return 2;
        }
        r.buf.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    }
    if (!std::freopen("/dev/null", "w", stdout)) return 2;
    std::vector<double> out;
    try {
        char magic[8];
        for (char& c : magic) c = r.get<char>();
        if (std::memcmp(magic, "FPREFC1", 8) != 0) throw std::runtime_error("bad magic");
        const int mode = r.get<int32_t>();
        const int rows = r.get<int32_t>(), cols = r.get<int32_t>();
        const double res = r.get<double>(), px = r.get<double>(), py = r.get<double>();
        if (rows <= 0 || cols <= 0 || rows > 4096 || cols > 4096) throw std::runtime_error("bad map size");
        grid_map_msgs::GridMap mapMsg;
        mapMsg.info.header.frame_id = "odom";
        mapMsg.info.resolution = res;
        mapMsg.info.length_x = static_cast<double>(rows) * res;
        mapMsg.info.length_y = static_cast<double>(cols) * res;
        mapMsg.info.pose.position.x = px;
        mapMsg.info.pose.position.y = py;
        mapMsg.rows = rows;
        mapMsg.cols = cols;
        mapMsg.layers = {"traversability", "elevation"};
        mapMsg.data.assign(2, std::vector<float>((size_t)rows * cols));
        for (int l = 0; l < 2; ++l)
            for (int i = 0; i < rows; ++i)
                for (int j = 0; j < cols; ++j) mapMsg.data[l][(size_t)i + (size_t)j * rows] = r.get<float>();
        std::vector<Param> params((size_t)r.get<int32_t>());
        for (Param& p : params) {
            p.key = r.str();
            p.kind = r.get<int32_t>();
            if (p.kind == 1)
                p.text = r.str();
            else
                p.value = r.get<double>();
        }

        if (mode == 0) {
            ros::NodeHandle nh;
            fillNode(nh, params);
            foothold_planner::FootholdPlanner planner(nh);
            nh.deliver<grid_map_msgs::GridMap>("/traversability_estimation/traversability_map", mapMsg);
            grid_map::GridMap map;  // the caller's own copy, as the by-value signatures take one
            if (!grid_map::GridMapRosConverter::fromMessage(mapMsg, map)) throw std::runtime_error("bad map message");
            const int n = r.get<int32_t>();
            for (int q = 0; q < n; ++q) {
                const int kind = r.get<int32_t>();
                grid_map::Position c(0, 0);
                c.x() = r.get<double>();
                c.y() = r.get<double>();
                const float footRadius = r.get<float>(), searchRadius = r.get<float>();
                double vx[4], vy[4];
                for (double& v : vx) v = r.get<double>();
                for (double& v : vy) v = r.get<double>();
                const size_t errors0 = ros::shimErrors().size();
                const unsigned long long oob0 = grid_map::oobReads();
                double rec[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                if (kind == 0) {
                    grid_map::Polygon polygon;
                    for (int k = 0; k < 4; ++k) polygon.addVertex(grid_map::Position(vx[k], vy[k]));
                    geometry_msgs::PointStamped result;
                    bool valid = false;
                    planner.checkFoothold(map, c, footRadius, searchRadius, polygon, result, valid);
                    const bool byDefault = planner.checkDefaultFoothold(map, c, footRadius);
                    rec[0] = valid;
                    rec[1] = byDefault ? 0 : (valid ? 1 : 2);
                    rec[2] = result.point.x;
                    rec[3] = result.point.y;
                    rec[4] = result.point.z;
                } else if (kind == 1) {
                    geometry_msgs::PointStamped query, result;
                    query.point.x = c.x();
                    query.point.y = c.y();
                    result.point.x = result.point.y = result.point.z = kNaN;  // stays NaN where no result is set
                    int beginRow = -1000000, endRow = -1000000;
                    planner.checkFootholdUseCentroidMethod(map, query, result, beginRow, endRow);  // the value it
                    rec[2] = result.point.x;  // returns is indeterminate on every path but the failed getSubmap
                    rec[3] = result.point.y;
                    rec[4] = result.point.z;
                    rec[5] = beginRow;
                    rec[6] = endRow;
                } else {
                    rec[4] = planner.getFootholdMeanHeight(map, c, footRadius, 0.01);
                }
                bool noMap = false;
                for (size_t e = errors0; e < ros::shimErrors().size(); ++e)
                    noMap = noMap || ros::shimErrors()[e] == "Can not get map.";
                rec[7] = noMap;
                rec[8] = (double)(grid_map::oobReads() - oob0);
                rec[9] = kind;
                out.insert(out.end(), rec, rec + 10);
            }
        } else {
            const int n = r.get<int32_t>();
            for (int q = 0; q < n; ++q) {
                const double x = r.get<double>(), y = r.get<double>(), z = r.get<double>();
                const int cycles = r.get<int32_t>();
                ros::NodeHandle nh;
                fillNode(nh, params);
                lfCurrentRow = g_lf0;  // the same entry state for every call, as one process serves them all
                rhCurrentRow = g_rh0;
                nlopt::callLog().clear();
                std::vector<Snapshot> snaps;
                nlopt::onOptimize() = [&snaps]() {
                    Snapshot s;
                    for (int k = 0; k < 8; ++k) {
                        s.nominal[k] = nominalIndex.at((size_t)k);
                        s.centroid[k] = centroidIndex.at((size_t)k);
                    }
                    s.lf = lfCurrentRow;
                    s.rh = rhCurrentRow;
                    snaps.push_back(s);
                };
                nh.setParam("initial_position/x", x);
                nh.setParam("initial_position/y", y);
                nh.setParam("initial_position/z", z);
                const unsigned long long oob0 = grid_map::oobReads();
                foothold_planner::FootholdPlanner planner(nh);
                nh.deliver<grid_map_msgs::GridMap>("/traversability_estimation/traversability_map", mapMsg);
                grid_map::GridMap parent;
                grid_map::GridMapRosConverter::fromMessage(mapMsg, parent);
                foothold_planner::GlobalFootholdPlan::Request req;
                foothold_planner::GlobalFootholdPlan::Response resp;
                req.gait_cycles = (uint8_t)cycles;
                const bool ret = nh.call("plan_global_footholds", req, resp);
                nlopt::onOptimize() = nullptr;
                const auto gaitMaps = nh.published<grid_map_msgs::GridMap>("gait_map");
                out.push_back(ret);
                out.push_back((double)gaitMaps.size());  // gates passed: where the call returned false, the failing cycle
                out.push_back((double)(grid_map::oobReads() - oob0));
                out.push_back((double)resp.footholds.footholds.size());
                pushTrack(out, nh, "global_footholds");
                pushTrack(out, nh, "global_footholds_centroid");
                pushTrack(out, nh, "global_footholds_opt");
                pushPath(out, nh, "nominal_feet_center_path");
                pushPath(out, nh, "centroid_feet_center_path");
                const auto& log = nlopt::callLog();
                out.push_back((double)log.size());
                for (size_t g = 0; g < log.size(); ++g) {
                    const nlopt::CallRecord& c = log[g];
                    grid_map::GridMap sub;
                    grid_map::GridMapRosConverter::fromMessage(gaitMaps.at(g), sub);
                    grid_map::Position corner;
                    grid_map::Index topLeft;
                    sub.getPosition(grid_map::Index(0, 0), corner);
                    parent.getIndex(corner, topLeft);
                    out.push_back(topLeft.x());
                    out.push_back(topLeft.y());
                    out.push_back(sub.getSize()(0));
                    out.push_back(sub.getSize()(1));
                    for (int k = 0; k < 8; ++k) out.push_back(snaps.at(g).nominal[k]);
                    for (int k = 0; k < 8; ++k) out.push_back(snaps.at(g).centroid[k]);
                    for (int k = 0; k < 8; ++k) out.push_back(c.lb.at((size_t)k));
                    for (int k = 0; k < 8; ++k) out.push_back(c.ub.at((size_t)k));
                    for (int k = 0; k < 8; ++k) out.push_back(c.x.at((size_t)k));
                    out.push_back(c.minf);
                    out.push_back(snaps.at(g).lf);
                    out.push_back(snaps.at(g).rh);
                    out.push_back(c.status);
                    out.push_back(c.nConstraints);
                }
            }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "ref_driver: %s\n", e.what());
        return 3;
    }
    std::ofstream o(argv[2], std::ios::binary);
    o.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(double)));
    return o ? 0 : 2;
}
