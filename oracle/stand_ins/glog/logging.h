// Stand-in for <glog/logging.h>, only as wide as the reference's corridor layer needs (oracle/Makefile, _ref/libref_corridor.so).
// This project's own text, written from glog's documented interface: LOG(severity) << ... is a stream that is dropped here,
// CHECK_LE(a, b) aborts the process when a > b, as glog's does.  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <cstdio>
#include <cstdlib>

namespace stand_in_glog {
struct NullStream {
    template <typename T>
    NullStream& operator<<(const T&) { return *this; }
};
}  // namespace stand_in_glog

#define LOG(severity) ::stand_in_glog::NullStream()
#define CHECK_LE(a, b)                                                                              \
    (((a) <= (b)) ? (void)0                                                                         \
                  : (std::fprintf(stderr, "Check failed: %s <= %s (%s:%d)\n", #a, #b, __FILE__, __LINE__), std::abort())), \
        ::stand_in_glog::NullStream()
