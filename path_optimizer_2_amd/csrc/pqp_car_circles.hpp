// pqp_car_circles.hpp - the car's circles and their placement, as the kernels of pqp_maps.hip (the footprint check), pqp_agents.hip (the
// agent check) and pqp_speed.hip (the path-time search) take them.  Device code only.  The function is forced inline and keeps fp
// contraction off: a fused multiply-add here breaks bit equality with the definition in include/pqp.h.
#pragma once

namespace pqp {

// The car's circles as the kernels take them, filled by car_circles_of (pqp_maps.hip) from a pqp_car_geometry.  rb is the broad phase's
// radius (pqp_agent_frames.hpp): the reference's own bounding circle (cr[6]) does not contain the corner circles, rb does.
struct CarCircles {
    double cx[7], cy[7], cr[7];      // vehicle frame: rr, rl, fr, fl, fm, rm, then the bounding circle (pqp_car_circles)
    double rb;                       // max_j (|c_j - c_6| + r_j): the six circles lie within rb of the bounding circle's centre
};

struct Point2 { double x, y; };

// local2Global(state, circle): x cos - y sin + ref.x, x sin + y cos + ref.y  (tools.cpp:51-52): one circle's centre (cx, cy) of the
// vehicle frame at the pose (x, y) with its heading's sine and cosine
__device__ __forceinline__ Point2 local_to_global(double cx, double cy, double sh, double ch, double x, double y) {
#pragma clang fp contract(off)
    return {cx * ch - cy * sh + x, cx * sh + cy * ch + y};
}

}  // namespace pqp
