/* Declared double of <pcl/filters/voxel_grid.h> -- NOT PCL and NOT a voxel grid.  filter() records a copy of its input
 * cloud (one entry per call, in call order) where the driver reads it, and passes the input through unchanged.  The
 * "/laser_cloud_less_flat" topic of a binary built with this double is therefore NOT the reference's and nothing may
 * compare it; the recorded filter INPUTS are what the reference's own text selected (scanRegistration.cpp:361-367). */
#pragma once
#include "pcl/point_cloud.h"

namespace pcl {

inline std::vector<std::vector<PointXYZI>> &ll_ref_voxel_inputs()
{
    static std::vector<std::vector<PointXYZI>> calls;
    return calls;
}

template <class PointT>
class VoxelGrid {
public:
    void setInputCloud(const typename PointCloud<PointT>::Ptr &cloud) { input_ = cloud; }
    void setLeafSize(float, float, float) {}
    void filter(PointCloud<PointT> &out)
    {
        ll_ref_voxel_inputs().push_back(input_->points);
        out = *input_;
    }
private:
    typename PointCloud<PointT>::Ptr input_;
};

}  // namespace pcl
