// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY.  nlopt::opt as the reference's opt track uses it (cpp:1116-1211), written
// from that usage.  NLopt's COBYLA STAYS UNPINNED: optimize() is the project's build-defined lattice rule
// (oracle/fpo_opt.cpp, "BUILD-DEFINED optimiser"), restated here so that it runs THROUGH THE REGISTERED CALLBACKS — the
// values it compares are the reference's own nloptFunc and nloptConstraint1..8, not the oracle's copies of them:
//   precondition: some lb > ub or the start x outside [lb, ub] -> std::invalid_argument (NLopt's C++ wrapper throws on
//             NLOPT_INVALID_ARGS; the reference swallows it, cpp:1224-1226), x untouched — status 1;
//   columns:  x[1], x[3], x[5], x[7], in that order, each set to the integer of its interval that minimises the
//             objective, others held (smallest integer on ties);
//   rows:     every integer point of the box of (x[0], x[2], x[4], x[6]) in lexicographic order, x[0] slowest; a point
//             is feasible when every registered constraint value is <= its tolerance; the winner is the first point
//             with the smallest key (violation, objective), violation = 0 when feasible and the largest constraint value
//             otherwise — status 0 when the winner is feasible, 2 when not;
//   more than 2^24 row points: x keeps the start rows with the new columns — status 3.
// The bounds are truncated to int as the oracle's are (the reference fills them from an Eigen::MatrixXi, cpp:1119-1127).
// Every optimize() call is appended to nlopt::callLog() — the driver reads the problems and solutions from it — and
// nlopt::onOptimize(), when set, runs first (the driver snapshots the reference's file-scope globals there).
#pragma once
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

namespace nlopt {

enum algorithm { LN_COBYLA, LN_BOBYQA, LN_NEWUOA, LN_NEWUOA_BOUND, LD_MMA, GN_ESCH, NUM_ALGORITHMS };
enum result { FAILURE = -1, INVALID_ARGS = -2, SUCCESS = 1, STOPVAL_REACHED = 2, FTOL_REACHED = 3, XTOL_REACHED = 4,
              MAXEVAL_REACHED = 5, MAXTIME_REACHED = 6 };
typedef double (*vfunc)(const std::vector<double>& x, std::vector<double>& grad, void* data);

struct CallRecord {
    std::vector<double> lb, ub, x0, x;
    double minf = 0.0;
    int status = 0;  // 0 feasible optimum, 1 precondition (thrown), 2 least violation, 3 too many points
    int nConstraints = 0;
};
inline std::vector<CallRecord>& callLog() {
    static std::vector<CallRecord> log;
    return log;
}
inline std::function<void()>& onOptimize() {
    static std::function<void()> f;
    return f;
}

class opt {
public:
    opt(algorithm a, unsigned n) : n_(n) { (void)a; }
    opt(const char* name, unsigned n) : n_(n) {
        static const char* known[] = {"LN_COBYLA", "LN_BOBYQA", "LN_NEWUOA", "LN_NEWUOA_BOUND", "LD_MMA", "GN_ESCH"};
        bool ok = false;
        for (const char* k : known) ok = ok || std::string(name) == k;
        if (!ok) throw std::invalid_argument(std::string("nlopt shim: unknown algorithm ") + name);
    }
    void set_lower_bounds(const std::vector<double>& v) { lb_ = v; }
    void set_upper_bounds(const std::vector<double>& v) { ub_ = v; }
    void set_min_objective(vfunc f, void* data) { f_ = f; fData_ = data; }
    void add_inequality_constraint(vfunc c, void* data, double tol = 0) { c_.push_back({c, data, tol}); }
    void remove_inequality_constraints() { c_.clear(); }
    void set_xtol_rel(double t) { xtolRel_ = t; }
    void set_initial_step(const std::vector<double>& dx) { dx_ = dx; }
    void get_initial_step(const std::vector<double>& x, std::vector<double>& dx) const {
        dx.assign(x.size(), 1.0);
        if (dx_.size() == x.size()) dx = dx_;
    }

    result optimize(std::vector<double>& x, double& minf) {
        if (onOptimize()) onOptimize()();
        callLog().emplace_back();
        CallRecord& rec = callLog().back();
        rec.lb = lb_; rec.ub = ub_; rec.x0 = x; rec.x = x;
        rec.nConstraints = (int)c_.size();
        if (x.size() != n_ || lb_.size() != n_ || ub_.size() != n_ || n_ != 8 || !f_) {
            rec.status = 1;
            throw std::invalid_argument("nlopt invalid argument");
        }
        std::vector<double> grad;
        rec.minf = f_(x, grad, fData_);
        std::vector<int> lo(n_), up(n_);
        for (unsigned k = 0; k < n_; ++k) {
            lo[k] = static_cast<int>(lb_[k]);
            up[k] = static_cast<int>(ub_[k]);
            if (lo[k] > up[k] || x[k] < lo[k] || x[k] > up[k]) {
                rec.status = 1;
                throw std::invalid_argument("nlopt invalid argument");
            }
        }
        std::vector<double> y = x;
        static const int cols[4] = {1, 3, 5, 7};
        for (int c = 0; c < 4; ++c) {
            const int k = cols[c];
            double best = 0.0;
            int bestV = lo[k];
            for (int v = lo[k]; v <= up[k]; ++v) {
                y[k] = v;
                const double f = f_(y, grad, fData_);
                if (v == lo[k] || f < best) {
                    best = f;
                    bestV = v;
                }
            }
            y[k] = bestV;
        }
        minf = f_(y, grad, fData_);
        double points = 1.0;
        for (unsigned k = 0; k < 8; k += 2) points *= static_cast<double>(up[k] - lo[k] + 1);
        if (points > static_cast<double>(1ll << 24)) {
            x = y;
            rec.x = x; rec.minf = minf; rec.status = 3;
            return MAXEVAL_REACHED;
        }
        bool found = false;
        double bestKey = 0.0, best = 0.0;
        double bx[4] = {y[0], y[2], y[4], y[6]};
        for (int a = lo[0]; a <= up[0]; ++a)
            for (int b = lo[2]; b <= up[2]; ++b)
                for (int c = lo[4]; c <= up[4]; ++c)
                    for (int d = lo[6]; d <= up[6]; ++d) {
                        y[0] = a; y[2] = b; y[4] = c; y[6] = d;
                        double key = 0.0;
                        if (!c_.empty()) {
                            bool feasible = true;
                            double resmax = 0.0;
                            for (const Constraint& q : c_) {
                                const double v = q.f(y, grad, q.data);
                                feasible = feasible && v <= q.tol;
                                resmax = v > resmax ? v : resmax;
                            }
                            key = feasible ? 0.0 : resmax;
                        }
                        const double f = f_(y, grad, fData_);
                        if (!found || key < bestKey || (key == bestKey && f < best)) {
                            found = true;
                            bestKey = key;
                            best = f;
                            bx[0] = a; bx[1] = b; bx[2] = c; bx[3] = d;
                        }
                    }
        y[0] = bx[0]; y[2] = bx[1]; y[4] = bx[2]; y[6] = bx[3];
        x = y;
        minf = best;
        rec.x = x; rec.minf = minf; rec.status = bestKey > 0.0 ? 2 : 0;
        return XTOL_REACHED;
    }

private:
    struct Constraint {
        vfunc f;
        void* data;
        double tol;
    };
    unsigned n_;
    std::vector<double> lb_, ub_, dx_;
    vfunc f_ = nullptr;
    void* fData_ = nullptr;
    std::vector<Constraint> c_;
    double xtolRel_ = 0.0;
};

}  // namespace nlopt
