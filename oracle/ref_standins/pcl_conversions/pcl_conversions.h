/* Declared double of <pcl_conversions/pcl_conversions.h> -- NOT pcl_conversions.  fromROSMsg reads x, y, z as three
 * consecutive floats at the start of every point_step-byte record (the driver builds exactly such messages, 12- or
 * 16-byte points); toROSMsg packs the points back to back.  No field tables, no endianness, no organised clouds. */
#pragma once
#include <cstring>
#include "pcl/point_cloud.h"
#include "sensor_msgs/PointCloud2.h"

namespace pcl {

inline void fromROSMsg(const sensor_msgs::PointCloud2 &msg, PointCloud<PointXYZ> &cloud)
{
    const std::size_t n = (std::size_t)msg.width * msg.height;
    cloud.points.resize(n);
    for (std::size_t i = 0; i < n; ++i) std::memcpy(&cloud.points[i], msg.data.data() + i * msg.point_step, 3 * sizeof(float));
    cloud.width = (std::uint32_t)n; cloud.height = 1;
}

template <class PointT>
void toROSMsg(const PointCloud<PointT> &cloud, sensor_msgs::PointCloud2 &msg)
{
    static_assert(sizeof(PointT) % sizeof(float) == 0, "packed float points");
    msg.height = 1; msg.width = (std::uint32_t)cloud.points.size();
    msg.point_step = (std::uint32_t)sizeof(PointT); msg.row_step = msg.point_step * msg.width;
    msg.data.resize(cloud.points.size() * sizeof(PointT));
    if (!cloud.points.empty()) std::memcpy(msg.data.data(), cloud.points.data(), msg.data.size());
}

}  // namespace pcl
