/* Declared double of <pcl/point_cloud.h> (+ removeNaNFromPointCloud of <pcl/filters/filter.h>) -- NOT PCL.
 * A point container with the members the reference's scan registration touches: points, size, push_back, +=, header,
 * width / height / is_dense.  removeNaNFromPointCloud drops a point when any of x, y, z is not finite and keeps the
 * order of the rest; that is this double's own statement and pins nothing about PCL's. */
#pragma once
#include <cmath>
#include "pcl/point_types.h"

namespace pcl {

struct PCLHeader { std::uint32_t seq = 0; std::uint64_t stamp = 0; };

template <class PointT>
class PointCloud {
public:
    typedef std::shared_ptr<PointCloud<PointT>> Ptr;
    typedef std::shared_ptr<const PointCloud<PointT>> ConstPtr;
    PCLHeader header;
    std::vector<PointT> points;
    std::uint32_t width = 0, height = 0;
    bool is_dense = true;

    std::size_t size() const { return points.size(); }
    void push_back(const PointT &p) { points.push_back(p); width = (std::uint32_t)points.size(); height = 1; }
    PointCloud &operator+=(const PointCloud &other)
    {
        points.insert(points.end(), other.points.begin(), other.points.end());
        width = (std::uint32_t)points.size(); height = 1;
        return *this;
    }
};

template <class PointT>
void removeNaNFromPointCloud(const PointCloud<PointT> &in, PointCloud<PointT> &out, std::vector<int> &index)
{
    std::vector<PointT> kept;
    index.clear();
    for (std::size_t i = 0; i < in.points.size(); ++i) {
        const PointT &p = in.points[i];
        if (std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z)) { kept.push_back(p); index.push_back((int)i); }
    }
    out.header = in.header;
    out.points.swap(kept);
    out.width = (std::uint32_t)out.points.size(); out.height = 1; out.is_dense = true;
}

}  // namespace pcl
