/* Declared double of <pcl/point_types.h> -- NOT PCL.  Only the two point structs that the reference's scan registration
 * names, as plain packed floats (PCL pads both to 16 bytes and adds SSE alignment; no arithmetic depends on that).
 * Used only by the recipe of oracle/ref.py, which compiles the reference's own source file against these doubles.
 * <algorithm> and <vector> come in here because the real header drags them in and the reference relies on that. */
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

namespace pcl {
struct PointXYZ { float x = 0.f, y = 0.f, z = 0.f; };
struct PointXYZI { float x = 0.f, y = 0.f, z = 0.f, intensity = 0.f; };
}  // namespace pcl
