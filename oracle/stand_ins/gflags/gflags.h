// Stand-in for <gflags/gflags.h>, only as wide as the reference's corridor layer needs (oracle/Makefile, _ref/libref_corridor.so).
// This project's own text, written from gflags' documented interface: DEFINE_type(name, default, help) defines a global FLAGS_name,
// DECLARE_type(name) declares it, google::RegisterFlagValidator registers a check that runs when a flag is parsed.  Nothing here
// parses a command line, so a validator is accepted and never called.  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <string>

#define DECLARE_double(name) extern double FLAGS_##name
#define DECLARE_bool(name) extern bool FLAGS_##name
#define DECLARE_string(name) extern std::string FLAGS_##name
#define DEFINE_double(name, value, help) double FLAGS_##name = (value)
#define DEFINE_bool(name, value, help) bool FLAGS_##name = (value)
#define DEFINE_string(name, value, help) std::string FLAGS_##name = (value)

namespace google {
template <typename Flag, typename Validator>
bool RegisterFlagValidator(const Flag*, Validator) { return true; }
}  // namespace google
