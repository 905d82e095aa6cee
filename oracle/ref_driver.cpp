/* Driver of the reference's scan registration node, for tests.  OUR text; it links the object that the recipe in
 * oracle/ref.py compiles from the reference's own scanRegistration.cpp (read in place, main renamed to
 * ll_ref_scan_registration_main) against the declared doubles of oracle/ref_standins/ and tests/native/ros_double/.
 *
 *   scanreg_<variant> IN OUT scan_line minimum_range lowerBound upBound
 *
 * IN : int32 n_scans, int32 floats_per_point (3 or 4); per scan: int32 n, n * floats_per_point float32.
 * OUT: int32 n_scans; per scan: int32 n_cloud, n_sharp, n_less_sharp, n_flat, n_voxel_calls; float32 laserCloud[n_cloud][4]
 *      ("/velodyne_cloud_2"), sharp, less_sharp, flat [..][4]; float32 cloudCurvature[0..n_cloud); int32
 *      cloudLabel[0..n_cloud); per VoxelGrid::filter call: int32 m, float32 input[m][4].
 * Every scan goes to the callback the node subscribed for "/rslidar_points", one after the other in ONE process, as the
 * node runs: the reference's arrays are globals that live on between scans.  "/laser_cloud_less_flat" is not written: with
 * the pass-through VoxelGrid double it is not the reference's. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "pcl/filters/voxel_grid.h"
#include "ros/ros.h"
#include "sensor_msgs/PointCloud2.h"

extern float cloudCurvature[400000];        /* globals with external linkage of the reference's translation unit */
extern int cloudLabel[400000];
int ll_ref_scan_registration_main(int argc, char **argv);

static void put(std::FILE *f, const void *p, std::size_t bytes)
{
    if (bytes && std::fwrite(p, 1, bytes, f) != bytes) { std::perror("ref_driver: write"); std::exit(3); }
}
static void get(std::FILE *f, void *p, std::size_t bytes)
{
    if (bytes && std::fread(p, 1, bytes, f) != bytes) { std::fprintf(stderr, "ref_driver: short input\n"); std::exit(3); }
}

static std::shared_ptr<sensor_msgs::PointCloud2> topic(const char *name, int expect_count)
{
    auto &D = ros::Double::get();
    if (D.count(name) != expect_count) { std::fprintf(stderr, "ref_driver: %s published %d times, expected %d\n", name, D.count(name), expect_count); std::exit(4); }
    return std::static_pointer_cast<sensor_msgs::PointCloud2>(D.latest(name));
}

int main(int argc, char **argv)
{
    if (argc != 7) { std::fprintf(stderr, "usage: %s IN OUT scan_line minimum_range lowerBound upBound\n", argv[0]); return 2; }
    auto &D = ros::Double::get();
    D.params_i["scan_line"] = std::atoi(argv[3]);
    D.params_d["minimum_range"] = std::atof(argv[4]);
    D.params_d["lowerBound"] = std::atof(argv[5]);
    D.params_d["upBound"] = std::atof(argv[6]);
    char name[] = "scanRegistration"; char *av[] = {name, nullptr};
    ll_ref_scan_registration_main(1, av);                   /* reads the parameters, subscribes, advertises; spin() returns at once */
    if (!D.callbacks.count("/rslidar_points")) { std::fprintf(stderr, "ref_driver: the node did not subscribe\n"); return 4; }
    auto handler = D.callbacks["/rslidar_points"];

    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("ref_driver: open"); return 3; }
    std::int32_t n_scans = 0, stride = 0;
    get(in, &n_scans, 4); get(in, &stride, 4);
    if (stride != 3 && stride != 4) { std::fprintf(stderr, "ref_driver: floats_per_point %d\n", stride); return 2; }
    put(out, &n_scans, 4);
    for (int s = 0; s < n_scans; ++s) {
        std::int32_t n = 0;
        get(in, &n, 4);
        auto msg = std::make_shared<sensor_msgs::PointCloud2>();
        msg->height = 1; msg->width = (std::uint32_t)n; msg->point_step = 4u * (std::uint32_t)stride; msg->row_step = msg->point_step * msg->width;
        msg->header.seq = (std::uint32_t)s; msg->header.frame_id = "rslidar";
        msg->data.resize((std::size_t)n * msg->point_step);
        get(in, msg->data.data(), msg->data.size());
        pcl::ll_ref_voxel_inputs().clear();
        handler(std::shared_ptr<const void>(msg));
        auto cloud = topic("/velodyne_cloud_2", s + 1);
        auto sharp = topic("/laser_cloud_sharp", s + 1), less_sharp = topic("/laser_cloud_less_sharp", s + 1), flat = topic("/laser_cloud_flat", s + 1);
        const auto &vox = pcl::ll_ref_voxel_inputs();
        std::int32_t head[5] = {(std::int32_t)cloud->width, (std::int32_t)sharp->width, (std::int32_t)less_sharp->width,
                                (std::int32_t)flat->width, (std::int32_t)vox.size()};
        if (cloud->point_step != 16 || head[0] > 400000) { std::fprintf(stderr, "ref_driver: unexpected laserCloud\n"); return 4; }
        put(out, head, sizeof head);
        put(out, cloud->data.data(), cloud->data.size());
        put(out, sharp->data.data(), sharp->data.size());
        put(out, less_sharp->data.data(), less_sharp->data.size());
        put(out, flat->data.data(), flat->data.size());
        put(out, cloudCurvature, (std::size_t)head[0] * 4);
        put(out, cloudLabel, (std::size_t)head[0] * 4);
        for (const auto &v : vox) {
            std::int32_t m = (std::int32_t)v.size();
            put(out, &m, 4);
            put(out, v.data(), v.size() * sizeof(pcl::PointXYZI));
        }
    }
    std::fclose(in);
    if (std::fclose(out) != 0) { std::perror("ref_driver: close"); return 3; }
    return 0;
}
