// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY.  Stand-ins for the handful of Eigen types the reference's planner
// touches, written from how FootholdPlanner.{hpp,cpp} uses them (Eigen itself is not available).
//
// SHIM-DEFINED CHOICE: every stand-in VALUE-INITIALISES TO ZERO.  Eigen leaves fixed and dynamic vectors
// uninitialised; the reference reads some of them before it writes them (a grid_map::Position after a failed
// getPosition, cpp:1702-1710, 1290-1314; Eigen::MatrixXi(2,4) entries on the paths that set no band, cpp:1003-1007).
// The oracle documents (0,0) / 0 for exactly those reads (fpo_planner.cpp, fpo_opt.cpp), so the shim makes the same
// choice instead of leaving the comparison to whatever the stack held.
#pragma once
#include <cstddef>
#include <ostream>
#include <vector>

namespace Eigen {

// Vector2d / Array2d / Vector2i / Array2i: two coefficients, x() y(), (k), (k, 0), [k].  transpose() returns the same
// two coefficients (the reference only streams it or converts it straight back, cpp:2051-2055, 2103, 2134).
template <class T>
struct Shim2 {
    T v[2] = {T(0), T(0)};
    Shim2() = default;
    Shim2(T a, T b) : v{a, b} {}
    T& x() { return v[0]; }
    T& y() { return v[1]; }
    const T& x() const { return v[0]; }
    const T& y() const { return v[1]; }
    T& operator()(int k) { return v[k]; }
    const T& operator()(int k) const { return v[k]; }
    T& operator()(int k, int) { return v[k]; }
    const T& operator()(int k, int) const { return v[k]; }
    T& operator[](int k) { return v[k]; }
    const T& operator[](int k) const { return v[k]; }
    Shim2 transpose() const { return *this; }
};
template <class T>
std::ostream& operator<<(std::ostream& os, const Shim2<T>& a) { return os << a.v[0] << " " << a.v[1]; }

using Vector2d = Shim2<double>;
using Array2d = Shim2<double>;
using Array2i = Shim2<int>;
using Vector2i = Shim2<int>;

struct Vector3d {
    double v[3] = {0, 0, 0};
    double& operator[](int k) { return v[k]; }
    const double& operator[](int k) const { return v[k]; }
    double& operator()(int k) { return v[k]; }
    const double& operator()(int k) const { return v[k]; }
};

// VectorXd(n) with the comma initialiser `v << a, b, c;` (cpp:666-670, 1344-1347) and [k] (cpp:3118 ff.).
class VectorXd {
public:
    VectorXd() = default;
    explicit VectorXd(int n) : d_((size_t)n, 0.0) {}
    double& operator[](int k) { return d_[(size_t)k]; }
    const double& operator[](int k) const { return d_[(size_t)k]; }
    double& operator()(int k) { return d_[(size_t)k]; }
    int size() const { return (int)d_.size(); }
    struct Comma {
        VectorXd& v;
        size_t k;
        Comma& operator,(double x) {
            v.d_.at(k++) = x;
            return *this;
        }
    };
    Comma operator<<(double x) {
        d_.at(0) = x;
        return Comma{*this, 1};
    }

private:
    std::vector<double> d_;
};

// MatrixXi(r, c): (i, j) only; assigning a double truncates toward zero as Eigen's int scalar does (cpp:1063-1075).
class MatrixXi {
public:
    MatrixXi() = default;
    MatrixXi(int r, int c) : r_(r), c_(c), d_((size_t)r * c, 0) {}
    int& operator()(int i, int j) { return d_.at((size_t)i + (size_t)j * r_); }
    const int& operator()(int i, int j) const { return d_.at((size_t)i + (size_t)j * r_); }
    int rows() const { return r_; }
    int cols() const { return c_; }

private:
    int r_ = 0, c_ = 0;
    std::vector<int> d_;
};

}  // namespace Eigen
