// C entry points around the reference's own corridor layer - tools.cpp, ReferencePath(Impl), CarGeometry, CollisionChecker, Map -
// compiled unchanged from where it lies by oracle/Makefile into oracle/_ref/libref_corridor.so, over the stand-in headers of
// oracle/stand_ins (gflags, glog, Eigen::Vector2d, grid_map::GridMap).  Everything above Map::getObstacleDistance is the
// reference's code; the grid lookup under it is the stand-in's restatement of grid_map (see stand_ins/grid_map_core).
// TEST INFRASTRUCTURE: tests/ref_corridor.py records what these calls return; nothing in the product links or loads this.
//
// Flat arrays throughout.  A state row is (s, k, heading, x, y), the layout of the path QP's reference states.  A bound row is
// f_lb f_ub r_lb r_ub c_lb c_ub f_x f_y r_x r_y: the first six in the order of pqp_corridor_bounds, then the front and rear centres.
// `car` is front_length, rear_length, car_width, safety_margin, enable_dynamic_segmentation: FLAGS_* are process globals, so every
// call that reads one sets them from `car` on entry and puts the reference's defaults back on return.
#include <cmath>
#include <memory>
#include <vector>

#include "config/planning_flags.hpp"
#include "data_struct/data_struct.hpp"
#include "data_struct/reference_path.hpp"
#include "tools/Map.hpp"
#include "tools/collosion_checker.hpp"
#include "tools/spline.h"
#include "tools/tools.hpp"

using namespace PathOptimizationNS;

namespace {

struct Line {
    tk::spline xs, ys;
};

struct Layer {
    grid_map::GridMap grid;
    std::unique_ptr<Map> map;
};

class Flags {
 public:
    explicit Flags(const double* car)
        : front_(FLAGS_front_length), rear_(FLAGS_rear_length), width_(FLAGS_car_width), margin_(FLAGS_safety_margin),
          dynamic_(FLAGS_enable_dynamic_segmentation) {
        FLAGS_front_length = car[0];
        FLAGS_rear_length = car[1];
        FLAGS_car_width = car[2];
        FLAGS_safety_margin = car[3];
        FLAGS_enable_dynamic_segmentation = car[4] != 0.0;
    }
    ~Flags() {
        FLAGS_front_length = front_;
        FLAGS_rear_length = rear_;
        FLAGS_car_width = width_;
        FLAGS_safety_margin = margin_;
        FLAGS_enable_dynamic_segmentation = dynamic_;
    }

 private:
    double front_, rear_, width_, margin_;
    bool dynamic_;
};

void put_state(const State& st, double* out) {
    out[0] = st.x; out[1] = st.y; out[2] = st.heading; out[3] = st.s;
}

void put_bound(const VehicleStateBound& b, double* out) {
    out[0] = b.front.lb; out[1] = b.front.ub; out[2] = b.rear.lb; out[3] = b.rear.ub; out[4] = b.center.lb; out[5] = b.center.ub;
    out[6] = b.front.x; out[7] = b.front.y; out[8] = b.rear.x; out[9] = b.rear.y;
}

// what both updateBounds calls leave behind: the kept states' bounds, their count, and the bound of isBlocked()
int put_bounds(const ReferencePath& path, double* bounds, int* blocked, double* blocked_row) {
    const auto& kept = path.getBounds();
    for (size_t i = 0; i < kept.size(); ++i) put_bound(kept[i], bounds + 10 * i);
    const auto hit = path.isBlocked();
    *blocked = hit ? 1 : 0;
    if (hit) put_bound(*hit, blocked_row);
    return static_cast<int>(kept.size());
}

}  // namespace

extern "C" {

void ref_flag_defaults(double* car) {
    car[0] = FLAGS_front_length; car[1] = FLAGS_rear_length; car[2] = FLAGS_car_width; car[3] = FLAGS_safety_margin;
    car[4] = FLAGS_enable_dynamic_segmentation ? 1.0 : 0.0;
}

void* ref_line_new(int m, const double* s, const double* x, const double* y) {
    Line* line = new Line();
    line->xs.set_points(std::vector<double>(s, s + m), std::vector<double>(x, x + m));
    line->ys.set_points(std::vector<double>(s, s + m), std::vector<double>(y, y + m));
    return line;
}
void ref_line_free(void* line) { delete static_cast<Line*>(line); }

// layer: column major, cell (ix, iy) at iy * rows + ix
void* ref_map_new(int rows, int cols, double resolution, double length_x, double length_y, double pos_x, double pos_y, const float* layer) {
    Layer* l = new Layer();
    l->grid.setGeometry(rows, cols, resolution, length_x, length_y, pos_x, pos_y);
    l->grid.add("distance", layer);
    l->map.reset(new Map(l->grid));
    return l;
}
void ref_map_free(void* layer) { delete static_cast<Layer*>(layer); }

// ---- tools.cpp ----------------------------------------------------------------------------------------------------------------
void ref_heading_curvature(void* line, int n, const double* s, double* heading, double* curvature) {
    const Line& l = *static_cast<Line*>(line);
    for (int i = 0; i < n; ++i) {
        heading[i] = getHeading(l.xs, l.ys, s[i]);
        curvature[i] = getCurvature(l.xs, l.ys, s[i]);
    }
}

// a [n][2], b [n][2] -> out [n]
void ref_distance(int n, const double* a, const double* b, double* out) {
    for (int i = 0; i < n; ++i) out[i] = distance(State(a[2 * i], a[2 * i + 1]), State(b[2 * i], b[2 * i + 1]));
}

// frame [n][3], target [n][3] (x, y, heading) -> out [n][3]; to_global: local2Global, else global2Local
void ref_transform(int n, int to_global, const double* frame, const double* target, double* out) {
    for (int i = 0; i < n; ++i) {
        const State f(frame[3 * i], frame[3 * i + 1], frame[3 * i + 2]), t(target[3 * i], target[3 * i + 1], target[3 * i + 2]);
        const State r = to_global ? local2Global(f, t) : global2Local(f, t);
        out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.heading;
    }
}

// the four projections: target [n][2] -> out [n][4] = x, y, heading, s of the returned State
void ref_projection(void* line, int n, const double* target, double max_s, double start_s, double* out) {
    const Line& l = *static_cast<Line*>(line);
    for (int i = 0; i < n; ++i) put_state(getProjection(l.xs, l.ys, target[2 * i], target[2 * i + 1], max_s, start_s), out + 4 * i);
}
void ref_projection_newton(void* line, int n, const double* target, double max_s, const double* hint_s, double* out) {
    const Line& l = *static_cast<Line*>(line);
    for (int i = 0; i < n; ++i) put_state(getProjectionByNewton(l.xs, l.ys, target[2 * i], target[2 * i + 1], max_s, hint_s[i]), out + 4 * i);
}
void ref_directional_projection(void* line, int n, const double* target, const double* angle, double max_s, double start_s, double* out) {
    const Line& l = *static_cast<Line*>(line);
    for (int i = 0; i < n; ++i)
        put_state(getDirectionalProjection(l.xs, l.ys, target[2 * i], target[2 * i + 1], angle[i], max_s, start_s), out + 4 * i);
}
void ref_directional_projection_newton(void* line, int n, const double* target, const double* angle, const double* max_s, const double* hint_s,
                                       double* out) {
    const Line& l = *static_cast<Line*>(line);
    for (int i = 0; i < n; ++i)
        put_state(getDirectionalProjectionByNewton(l.xs, l.ys, target[2 * i], target[2 * i + 1], angle[i], max_s[i], hint_s[i]), out + 4 * i);
}

// ---- ReferencePath ------------------------------------------------------------------------------------------------------------
// setSpline + buildReferenceFromSpline, then updateBounds (d_heading null) or updateBoundsOnInputStates on n_input states that carry
// d_heading[i].  states [cap][5] gets the states as built (before either call trims them), bounds [cap][10] the kept ones' bounds.
// Returns the number of states built (nothing is written where it exceeds cap), -1 where buildReferenceFromSpline returns false.
// layer null: build only.
int ref_corridor(void* line, double max_s, double ds_small, double ds_large, const double* car, void* layer, int n_input, const double* d_heading,
                 int cap, double* states, double* bounds, int* kept, int* blocked, double* blocked_row) {
    const Line& l = *static_cast<Line*>(line);
    Flags flags(car);
    ReferencePath path;
    path.setSpline(l.xs, l.ys, max_s);
    *kept = 0; *blocked = 0;
    if (!path.buildReferenceFromSpline(ds_small, ds_large)) return -1;
    const int n = static_cast<int>(path.getSize());
    if (n > cap) return n;
    const auto& built = path.getReferenceStates();
    for (int i = 0; i < n; ++i) {
        double* o = states + 5 * i;
        o[0] = built[i].s; o[1] = built[i].k; o[2] = built[i].heading; o[3] = built[i].x; o[4] = built[i].y;
    }
    if (!layer) return n;
    const Map& map = *static_cast<Layer*>(layer)->map;
    if (d_heading) {
        std::vector<SlState> input(n_input);
        for (int i = 0; i < n_input; ++i) input[i].d_heading = d_heading[i];
        path.updateBoundsOnInputStates(map, input);
    } else {
        path.updateBounds(map);
    }
    *kept = put_bounds(path, bounds, blocked, blocked_row);
    return n;
}

// getClearanceWithDirectionStrict at arbitrary states, state [n][3] = x, y, heading -> out [n][2] = lb, ub.  The function is private;
// it is reached through the public calls: buildReferenceFromStates on three copies of the state (a spline needs three knots) and
// updateBounds, whose centre bound of the first state - kept, or left in isBlocked() where the front or rear bound closed - is it.
void ref_clearance(int n, const double* state, const double* car, void* layer, double* out) {
    Flags flags(car);
    const Map& map = *static_cast<Layer*>(layer)->map;
    for (int i = 0; i < n; ++i) {
        std::vector<State> three;
        for (int k = 0; k < 3; ++k) three.emplace_back(state[3 * i], state[3 * i + 1], state[3 * i + 2], 0.0, static_cast<double>(k));
        ReferencePath path;
        path.buildReferenceFromStates(three);
        path.updateBounds(map);
        const auto& kept = path.getBounds();
        const auto hit = path.isBlocked();
        const VehicleStateBound::SingleBound& c = kept.empty() ? hit->center : kept[0].center;
        out[2 * i] = c.lb; out[2 * i + 1] = c.ub;
    }
}

// ---- CarGeometry, CollisionChecker, Map -----------------------------------------------------------------------------------------
// state [n][3] = x, y, heading.  circles [n][7][3]: getCircles' six, then getBoundingCircle, of the checker's car
// (collision_checker.cpp:9-14); free_circles / free_bounding [n]: isSingleStateCollisionFree / ...Improved
void ref_footprint(int n, const double* state, const double* car, void* layer, double* circles, unsigned char* free_circles,
                   unsigned char* free_bounding) {
    Flags flags(car);
    const CarGeometry geometry(FLAGS_car_width, fabs(FLAGS_rear_length), FLAGS_front_length);
    CollisionChecker checker(static_cast<Layer*>(layer)->grid);
    for (int i = 0; i < n; ++i) {
        const State st(state[3 * i], state[3 * i + 1], state[3 * i + 2]);
        const auto six = geometry.getCircles(st);
        double* o = circles + 21 * i;
        for (size_t k = 0; k < 6; ++k) { o[3 * k] = six[k].x; o[3 * k + 1] = six[k].y; o[3 * k + 2] = six[k].r; }
        const Circle big = geometry.getBoundingCircle(st);
        o[18] = big.x; o[19] = big.y; o[20] = big.r;
        free_circles[i] = checker.isSingleStateCollisionFree(st) ? 1 : 0;
        free_bounding[i] = checker.isSingleStateCollisionFreeImproved(st) ? 1 : 0;
    }
}

// point [n][2] -> distance [n] (Map::getObstacleDistance), inside [n] (Map::isInside)
void ref_obstacle_distance(void* layer, int n, const double* point, double* distance, unsigned char* inside) {
    const Map& map = *static_cast<Layer*>(layer)->map;
    for (int i = 0; i < n; ++i) {
        const Eigen::Vector2d p(point[2 * i], point[2 * i + 1]);
        distance[i] = map.getObstacleDistance(p);
        inside[i] = map.isInside(p) ? 1 : 0;
    }
}

}  // extern "C"
