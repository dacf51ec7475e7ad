// carver.hpp — what the staging of every step-preparation call shares (step_prep.cpp, hdv_call_host.hpp): the regions of one block, and
// poses as the kernels read them.  Host only, no HIP header.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

// Hands out the regions of one block in the order they are asked for.  A region starts at a multiple of its element's alignment
// (or of `align`); the offsets hold for the pinned staging block and for the device workspace alike.
struct Carver {
    size_t at = 0;  // the first free byte: after the last region, the size of the block so far
    template <class T>
    size_t take(size_t count, size_t align = alignof(T)) {
        at = (at + align - 1) & ~(align - 1);
        const size_t offset = at;
        at += count * sizeof(T);
        return offset;
    }
    size_t end8() { return take<unsigned char>(0, 8); }  // the size so far, rounded up to 8
};

// poses as the kernels read them: x, y, cos_yaw, sin_yaw of m poses one array after the other, and the trims 0-based
inline void stage_poses(double* in, size_t m, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw, int32_t* trim0 = nullptr,
                        const int32_t* trim = nullptr) {
    std::memcpy(in, x, m * sizeof(double));
    std::memcpy(in + m, y, m * sizeof(double));
    std::memcpy(in + 2 * m, cos_yaw, m * sizeof(double));
    std::memcpy(in + 3 * m, sin_yaw, m * sizeof(double));
    if (trim0)
        for (size_t v = 0; v < m; ++v) trim0[v] = trim[v] - 1;
}
