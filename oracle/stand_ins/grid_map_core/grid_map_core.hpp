// Stand-in for <grid_map_core/grid_map_core.hpp>, only as wide as the reference's corridor layer needs (oracle/Makefile,
// _ref/libref_corridor.so): a GridMap with ONE float layer, exists / isInside / atPosition(layer, position, INTER_LINEAR).
//
// THIS IS A RESTATEMENT, NOT THE LIBRARY.  grid_map (ANYbotics/grid_map) is third-party, neither in this repository nor in the
// reference tree.  What is written here is this project's own text, from grid_map_core 1.6.x's published behaviour
// (GridMapMath.cpp: checkIfPositionWithinMap, getIndexFromPosition, getPositionFromIndex, getLinearIndexFromIndex;
// GridMap.cpp: atPosition, atPositionLinearInterpolated), and it is the same set of conventions that oracle/corridor_oracle.py
// states in Python: grid_is_inside, grid_index, grid_cell_position, grid_at_linear and the nearest-cell fall-back of
// obstacle_distance.  tests/test_ref_corridor.py holds the two to each other bit for bit; neither has been held to grid_map
// itself.  Everything ABOVE Map::getObstacleDistance in libref_corridor.so is the reference's own code; this lookup is not.
// TEST INFRASTRUCTURE ONLY.
#pragma once
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

#include "Eigen/Core"

namespace grid_map {

typedef Eigen::Vector2d Position;

enum class InterpolationMethods { INTER_NEAREST, INTER_LINEAR };

class GridMap {
 public:
    GridMap() = default;

    // rows: cells along x, cols: cells along y; data: the layer in column-major order (cell (ix, iy) at iy * rows + ix); a map
    // that was never moved (start index 0).  Cell (0, 0) is the +x / +y corner, indices grow towards -x / -y.
    void setGeometry(int rows, int cols, double resolution, double length_x, double length_y, double pos_x, double pos_y) {
        rows_ = rows; cols_ = cols; resolution_ = resolution;
        length_[0] = length_x; length_[1] = length_y;
        pos_[0] = pos_x; pos_[1] = pos_y;
    }
    void add(const std::string& layer, const float* data) {
        layer_ = layer;
        data_.assign(data, data + static_cast<std::size_t>(rows_) * static_cast<std::size_t>(cols_));
    }

    bool exists(const std::string& layer) const { return !data_.empty() && layer == layer_; }

    // checkIfPositionWithinMap: -(p - c - L / 2) in [0, L)
    bool isInside(const Position& p) const {
        const double tx = -(p.x() - pos_[0] - 0.5 * length_[0]);
        const double ty = -(p.y() - pos_[1] - 0.5 * length_[1]);
        return tx >= 0.0 && ty >= 0.0 && tx < length_[0] && ty < length_[1];
    }

    // INTER_LINEAR falls back to the nearest cell where a neighbour is missing, as GridMap::atPosition does
    float atPosition(const std::string&, const Position& p, InterpolationMethods method = InterpolationMethods::INTER_NEAREST) const {
        float value;
        if (method == InterpolationMethods::INTER_LINEAR && linear(p, value)) return value;
        int ix, iy;
        index(p, ix, iy);
        if (ix < 0 || iy < 0 || ix >= rows_ || iy >= cols_) return std::nanf("");      // (upstream would read outside the buffer)
        return data_[static_cast<std::size_t>(iy) * rows_ + ix];
    }

 private:
    // getIndexFromPosition: (p - L / 2 - c) / resolution truncated toward zero, negated
    void index(const Position& p, int& ix, int& iy) const {
        const double vx = (p.x() - 0.5 * length_[0] - pos_[0]) / resolution_;
        const double vy = (p.y() - 0.5 * length_[1] - pos_[1]) / resolution_;
        ix = -static_cast<int>(vx);
        iy = -static_cast<int>(vy);
    }
    // getPositionFromIndex: c + (L / 2 - resolution / 2) + resolution * (-index)
    void cell(int ix, int iy, double& x, double& y) const {
        const double ox = 0.5 * length_[0] - 0.5 * resolution_;
        const double oy = 0.5 * length_[1] - 0.5 * resolution_;
        x = (pos_[0] + ox) + resolution_ * static_cast<double>(-ix);
        y = (pos_[1] + oy) + resolution_ * static_cast<double>(-iy);
    }
    // atPositionLinearInterpolated: the four cells round the position, tested by their LINEAR index only (as size_t, so a
    // negative one wraps): a neighbour with ix = -1 and iy >= 1 passes and reads the element that index points at.  An index
    // equal to the layer's size is refused here (upstream's test is `>`, which would read one past the buffer).
    bool linear(const Position& p, float& value) const {
        int i0[2];
        index(p, i0[0], i0[1]);
        double cx, cy;
        cell(i0[0], i0[1], cx, cy);
        int idx[4][2] = {{i0[0], i0[1]}, {0, 0}, {0, 0}, {0, 0}};
        bool dir;
        int shift[4];
        if (p.x() >= cx) { idx[1][0] = i0[0] - 1; idx[1][1] = i0[1]; dir = true; }
        else             { idx[1][0] = i0[0] + 1; idx[1][1] = i0[1]; dir = false; }
        if (p.y() >= cy) {
            idx[2][0] = i0[0]; idx[2][1] = i0[1] - 1;
            if (dir) { shift[0] = 0; shift[1] = 1; shift[2] = 2; shift[3] = 3; }
            else     { shift[0] = 1; shift[1] = 0; shift[2] = 3; shift[3] = 2; }
        } else {
            idx[2][0] = i0[0]; idx[2][1] = i0[1] + 1;
            if (dir) { shift[0] = 2; shift[1] = 3; shift[2] = 0; shift[3] = 1; }
            else     { shift[0] = 3; shift[1] = 2; shift[2] = 1; shift[3] = 0; }
        }
        idx[3][0] = idx[1][0]; idx[3][1] = idx[2][1];
        const std::size_t end_lin = static_cast<std::size_t>(rows_) * static_cast<std::size_t>(cols_);
        double f[4];
        for (int k = 0; k < 4; ++k) {
            const int* c = idx[shift[k]];
            const std::size_t lin = static_cast<std::size_t>(static_cast<long long>(c[1]) * rows_ + c[0]);
            if (lin >= end_lin) return false;
            f[k] = static_cast<double>(data_[lin]);
        }
        double qx, qy;
        cell(idx[shift[0]][0], idx[shift[0]][1], qx, qy);
        const double rx = (p.x() - qx) / resolution_;
        const double ry = (p.y() - qy) / resolution_;
        const double fx = 1.0 - rx;
        const double fy = 1.0 - ry;
        value = static_cast<float>(f[0] * fx * fy + f[1] * rx * fy + f[2] * fx * ry + f[3] * rx * ry);
        return true;
    }

    int rows_ = 0, cols_ = 0;
    double resolution_ = 1.0;
    double length_[2] = {0.0, 0.0};
    double pos_[2] = {0.0, 0.0};
    std::string layer_;
    std::vector<float> data_;
};

}  // namespace grid_map
