// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY.  grid_map_core as the reference's FootholdPlanner uses it, written from
// that usage.  grid_map_core's SEMANTICS STAY UNPINNED: every piece of index / position arithmetic and every iterator
// order here forwards to oracle/fpo_gridmap.hpp, so the project keeps ONE statement of them and not a second
// recollection.  What this header adds is only the API surface (named layers, Eigen-like accessors).
//
// SHIM-DEFINED CHOICES (stated, because upstream leaves them undefined):
//   * Position, Index, Length, Size value-initialise to zero (shim/eigen.hpp);
//   * at() / isValid() with an index outside the layer — the reference's row scan reads (row, size(1)), one column past
//     the layer, in every row it scans (cpp:1719-1736; with Eigen's column-major storage that is rows*cols + row, past
//     the allocation) — return NaN / false and COUNT the access (oobReads()), instead of reading foreign memory.  NaN
//     compares false against the threshold, i.e. the cell is not counted: what the oracle's in-bounds scan does.
#pragma once
#include <atomic>
#include <cmath>
#include <limits>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../fpo_gridmap.hpp"
#include "../shim/eigen.hpp"

namespace grid_map {

using Position = Eigen::Vector2d;
using Length = Eigen::Array2d;
using Index = Eigen::Array2i;
using Size = Eigen::Array2i;

inline fpo::Vec2 toFpo(const Position& p) { return {p.x(), p.y()}; }
inline fpo::Idx2 toFpo(const Index& i) { return {i.x(), i.y()}; }

inline std::atomic<unsigned long long>& oobReadCounter() {
    static std::atomic<unsigned long long> n{0};
    return n;
}
inline unsigned long long oobReads() { return oobReadCounter().load(); }

// A view of one layer (column-major f32, as Eigen::MatrixXf): (linear) and (row, col).
class Matrix {
public:
    Matrix() = default;
    Matrix(std::vector<float>* d, int rows, int cols) : d_(d), rows_(rows), cols_(cols) {}
    float& operator()(int k) { return d_->at((size_t)k); }
    float& operator()(int i, int j) { return d_->at((size_t)i + (size_t)j * rows_); }
    int rows() const { return rows_; }
    int cols() const { return cols_; }

private:
    std::vector<float>* d_ = nullptr;
    int rows_ = 0, cols_ = 0;
};

class GridMap {
public:
    GridMap() = default;
    // the driver's side: a canonical map (start index 0) with the two layers the reference reads
    GridMap(const fpo::GridMap& g, const std::string& frame) : g_(g), frame_(frame) {}
    const fpo::GridMap& geometry() const { return g_; }

    const Position getPosition() const { return Position(g_.position.x, g_.position.y); }
    const Length getLength() const { return Length(g_.length.x, g_.length.y); }
    const Size getSize() const { return Size(g_.size.i, g_.size.j); }
    double getResolution() const { return g_.res; }
    const std::string& getFrameId() const { return frame_; }
    void setFrameId(const std::string& f) { frame_ = f; }
    std::vector<std::string> getLayers() const {
        std::vector<std::string> l{"traversability"};
        if (!g_.elev.empty()) l.push_back("elevation");
        return l;
    }

    bool getPosition(const Index& index, Position& position) const {
        fpo::Vec2 p = toFpo(position);
        const bool ok = g_.getPosition(toFpo(index), p);  // writes only on success, as upstream
        if (ok) position = Position(p.x, p.y);
        return ok;
    }
    bool getIndex(const Position& position, Index& index) const {
        fpo::Idx2 i;
        const bool ok = g_.getIndex(toFpo(position), i);  // the index is written even when outside
        index = Index(i.i, i.j);
        return ok;
    }
    GridMap getSubmap(const Position& position, const Length& length, bool& isSuccess) const {
        GridMap sub;
        sub.g_ = g_.getSubmap(toFpo(position), {length.x(), length.y()}, isSuccess, nullptr, true);
        sub.frame_ = frame_;
        return sub;
    }

    Matrix& operator[](const std::string& layer) {
        view_ = Matrix(&store(layer), g_.size.i, g_.size.j);
        return view_;
    }
    float at(const std::string& layer, const Index& index) const {
        const std::vector<float>& d = const_cast<GridMap*>(this)->store(layer);
        if (!fpo::checkIfIndexInRange(toFpo(index), g_.size)) {
            ++oobReadCounter();
            return std::numeric_limits<float>::quiet_NaN();
        }
        return d.at((size_t)index.x() + (size_t)index.y() * g_.size.i);
    }
    bool isValid(const Index& index, const std::string& layer) const { return fpo::GridMap::isValid(at(layer, index)); }

private:
    std::vector<float>& store(const std::string& layer) {
        if (layer == "traversability") return g_.trav;
        if (layer == "elevation" && !g_.elev.empty()) return g_.elev;
        throw std::out_of_range("GridMap shim: no layer '" + layer + "'");
    }
    fpo::GridMap g_;
    std::string frame_;
    Matrix view_;
    friend class GridMapRosConverter;
};

// ---- iterators: thin wrappers of oracle/fpo_gridmap.hpp's ---------------------------------------------
class CircleIterator {
public:
    CircleIterator(const GridMap& map, const Position& center, double radius) : it_(map.geometry(), toFpo(center), radius) {}
    bool isPastEnd() const { return it_.isPastEnd(); }
    CircleIterator& operator++() { ++it_; return *this; }
    Index operator*() const { const fpo::Idx2 i = *it_; return Index(i.i, i.j); }

private:
    fpo::CircleIterator it_;
};
class SpiralIterator {
public:
    SpiralIterator(const GridMap& map, const Position& center, double radius) : it_(map.geometry(), toFpo(center), radius) {}
    bool isPastEnd() const { return it_.isPastEnd(); }
    SpiralIterator& operator++() { ++it_; return *this; }
    Index operator*() const { const fpo::Idx2 i = *it_; return Index(i.i, i.j); }

private:
    fpo::SpiralIterator it_;
};
class LineIterator {
public:
    LineIterator(const GridMap&, const Index& start, const Index& end) : it_(toFpo(start), toFpo(end)) {}
    bool isPastEnd() const { return it_.isPastEnd(); }
    LineIterator& operator++() { ++it_; return *this; }
    Index operator*() const { const fpo::Idx2 i = *it_; return Index(i.i, i.j); }

private:
    fpo::LineIterator it_;
};
class GridMapIterator {
public:
    explicit GridMapIterator(const GridMap& map) : it_(map.geometry().size) {}
    bool isPastEnd() const { return it_.isPastEnd(); }
    GridMapIterator& operator++() { ++it_; return *this; }
    Index operator*() const { const fpo::Idx2 i = *it_; return Index(i.i, i.j); }
    int getLinearIndex() const { return (int)it_.linearIndex(); }

private:
    fpo::GridMapIterator it_;
};

// ---- Polygon: vertices + isInside of fpo::Polygon ---------------------------------------------------------
class Polygon {
public:
    void addVertex(const Position& v) { p_.addVertex(toFpo(v)); }
    void setFrameId(const std::string& f) { frame_ = f; }
    const std::string& getFrameId() const { return frame_; }
    bool isInside(const Position& point) const { return p_.isInside(toFpo(point)); }
    const std::vector<fpo::Vec2>& vertices() const { return p_.vertices; }
    // only streamed under debug2_ (cpp:2385): the vertex mean, shim-defined
    Position getCentroid() const {
        Position c;
        for (const fpo::Vec2& v : p_.vertices) { c.x() += v.x; c.y() += v.y; }
        if (!p_.vertices.empty()) { c.x() /= (double)p_.vertices.size(); c.y() /= (double)p_.vertices.size(); }
        return c;
    }

private:
    fpo::Polygon p_;
    std::string frame_;
};

}  // namespace grid_map
