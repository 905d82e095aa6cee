/*
 * lightloam_host.hpp -- C++ host-side mirror of the reference's own seams over the C ABI (lightloam_hip.h).
 *
 * The reference (BrenYi/Light-LOAM, paths relative to /root/reference/) is three ROS1 nodes; a maintainer replaces
 * the BODY of the functions below and keeps names, argument meaning, output order and error behaviour:
 *   laserCloudHandler                           src/scanRegistration.cpp:87-428
 *   graph_based_correspondence_vote_simple      src/laserOdometry.cpp:165-342 (call :796)
 *   the correspondence loops + ceres::Solve     src/laserOdometry.cpp:439-832  -> OdometryFrame below
 *   Corre_Match / Vertex_Vote / compare_score   include/aloam_velodyne/common.h:20-52
 * Header-only, C++14, no ROS / PCL / Eigen / Ceres needed (this image has none): clouds are std::vector<PointXYZI>
 * with the PCL field names; templates convert from any point type that has x, y, z (and intensity).
 * The optional Ceres adapter at the end compiles only when <ceres/ceres.h> is available and is NOT compiled or
 * tested in this image.
 */
#ifndef LIGHTLOAM_HOST_HPP
#define LIGHTLOAM_HOST_HPP

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "lightloam_hip.h"

namespace lightloam {

struct PointXYZI { float x, y, z, intensity; };                      /* pcl::PointXYZI without the SSE padding */
static_assert(sizeof(PointXYZI) == sizeof(ll_point), "layout");
typedef PointXYZI PointType;                                          /* common.h:7 */
typedef ll_pose_info PoseInfo;                                        /* the measured information of a scan-to-map solve (lightloam_hip.h) */

typedef struct {                                                      /* common.h:20-31 */
    int index;
    PointXYZI src;
    PointXYZI tgt;
    float score;
    float s;
} Corre_Match;

typedef struct { int index; float score; } Vertex_Vote;               /* common.h:40-43 */
struct compare_score { bool operator()(Vertex_Vote const &a, Vertex_Vote const &b) { return a.score > b.score; } };   /* :50-52 */

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

/* RAII ll_ctx; one per node thread (the reference nodes are single-threaded spinners, scanRegistration.cpp:475) */
class Context {
public:
    /* distortion: the DISTORTION macro of laserOdometry.cpp:23 (0 in the reference's build; 1 = its per-point interpolation path) */
    /* max_ring_points: capacity of one scan line (0: the library default, 2304 = a 2048-column sensor; real HDL-64E / KITTI data
     * under the linear 64-ring model of scanRegistration.cpp:162 needs 4608 -- some bins hold two lasers) */
    explicit Context(int scan_line, int batch = 2, int device = 0, double minimum_range = -1.0,
                     float lowerBound = -24.9f, float upBound = 2.0f, int distortion = 0, int max_ring_points = 0, int input_stride_floats = 4) {
        ll_default_params(&p_, scan_line);
        p_.batch = batch;
        p_.distortion = distortion;
        p_.input_stride_floats = input_stride_floats;                           /* 3: the resident scan keeps x, y, z only, as pcl::fromROSMsg into PointXYZ does (:105-106) */
        if (max_ring_points > 0) p_.max_ring_points = max_ring_points;
        if (minimum_range >= 0) p_.minimum_range = (float)minimum_range;       /* nh.param("minimum_range") :438 */
        p_.lower_bound = lowerBound; p_.up_bound = upBound;                     /* nh.param("lowerBound" / "upBound") :439-440 */
        const int rc = ll_create(device, &p_, &ctx_);
        if (rc != LL_OK) throw Error(rc, ll_last_error(nullptr));               /* LL_ERR_BAD_RINGS == "only support velodyne with 16, 32 or 64 scan line" :447-451 */
    }
    ~Context() { ll_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    ll_ctx *get() const { return ctx_; }
    const ll_params &params() const { return p_; }
    void check(int rc) const { if (rc != LL_OK) throw Error(rc, ll_last_error(ctx_)); }
    /* TransformToEnd (laserOdometry.cpp:99-114; the reference's call sits under `if (0)`, :861) in the frame loops -- odometry_frames,
     * Drives --: 0 off (default), 1 the solved frames' less-sharp / less-flat clouds are re-projected to the end of their sweep in place,
     * 2 also laserCloud.  Needs distortion = 1 (Error LL_ERR_STATE otherwise). */
    void set_deskew(int mode) { check(ll_set_deskew(ctx_, mode)); }
    /* the stage on its own: slots [first, first + count) with pose7 ([count][7]; nullptr = the poses the slots hold on the device), then
     * their search grids anew.  A slot takes it once per extraction / upload (Error LL_ERR_STATE for a second one). */
    void deskew_slots(int first, int count, const double *pose7 = nullptr, int mode = 1) { check(ll_deskew_slots(ctx_, first, count, pose7, mode)); }
private:
    ll_params p_;
    ll_ctx *ctx_ = nullptr;
};

/* ---- scanRegistration.cpp:87-428.  Input: the points of the PointCloud2 message (x,y,z[,.]) with `stride` floats
 * per point; outputs: what the node publishes on /velodyne_cloud_2, /laser_cloud_sharp, /laser_cloud_less_sharp,
 * /laser_cloud_flat, /laser_cloud_less_flat (:382-410), same point order.  Returns false where the reference would
 * have dereferenced an empty cloud (no point survives the filters). */
inline bool laserCloudHandler(Context &c, int slot, const float *xyz, int stride, int n,
                              std::vector<PointXYZI> &laserCloud, std::vector<PointXYZI> &cornerPointsSharp,
                              std::vector<PointXYZI> &cornerPointsLessSharp, std::vector<PointXYZI> &surfPointsFlat,
                              std::vector<PointXYZI> &surfPointsLessFlat)
{
    c.check(ll_upload_scan(c.get(), slot, xyz, stride, n));
    c.check(ll_extract_batch(c.get(), slot, 1));
    ll_scan_info info;
    c.check(ll_get_scan_info(c.get(), slot, &info));
    if (info.status == LL_ERR_EMPTY) return false;
    if (info.status != LL_OK) throw Error(info.status, "scan registration failed (capacity)");
    laserCloud.resize(info.n); cornerPointsSharp.resize(info.n_sharp); cornerPointsLessSharp.resize(info.n_less_sharp);
    surfPointsFlat.resize(info.n_flat); surfPointsLessFlat.resize(info.n_less_flat);
    c.check(ll_download_cloud(c.get(), slot, (ll_point *)laserCloud.data(), info.n, nullptr, nullptr));
    c.check(ll_download_features(c.get(), slot, (ll_point *)cornerPointsSharp.data(), info.n_sharp,
                                 (ll_point *)cornerPointsLessSharp.data(), info.n_less_sharp,
                                 (ll_point *)surfPointsFlat.data(), info.n_flat, (ll_point *)surfPointsLessFlat.data(), info.n_less_flat));
    return true;
}

/* ---- laserOdometry.cpp:165-342, same signature minus the six unused arguments.  Appends to selected_idx in the
 * reference's order: per region, the vote records sorted with the SAME std::sort / compare_score call on the same
 * initial sequence, then walked from the low-count end (:255, :304-329). */
inline void graph_based_correspondence_vote_simple(Context &c, std::vector<Corre_Match> &correspondences, bool corner_case,
                                                   std::vector<Vertex_Vote> &selected_idx)
{
    const int n = (int)correspondences.size();
    if (n == 0) return;
    std::vector<ll_point> src(n), tgt(n);
    for (int i = 0; i < n; ++i) {
        src[i] = {correspondences[i].src.x, correspondences[i].src.y, correspondences[i].src.z, correspondences[i].src.intensity};
        tgt[i] = {correspondences[i].tgt.x, correspondences[i].tgt.y, correspondences[i].tgt.z, correspondences[i].tgt.intensity};
    }
    std::vector<int> count(n);
    c.check(ll_vote_host(c.get(), src.data(), tgt.data(), n, corner_case ? 1 : 0, count.data(), nullptr, nullptr));
    const int number_of_region = corner_case ? 5 : 10;                                  /* :179-188 */
    for (int num_region = 0; num_region < number_of_region; num_region++) {
        const int initial_pos = n / number_of_region * num_region;                      /* :202 */
        const int end_pos = (num_region == number_of_region - 1) ? n : n / number_of_region * (num_region + 1);
        const int cor_size = end_pos - initial_pos;
        std::vector<Vertex_Vote> vote_record((size_t)std::max(cor_size, 0));
        for (int i = 0; i < cor_size; ++i) { vote_record[i].index = i; vote_record[i].score = (float)count[initial_pos + i]; }
        std::sort(vote_record.begin(), vote_record.end(), compare_score());             /* :255 */
        const float num_selected = 0.90f * cor_size;                                    /* :299-300 */
        for (int i = cor_size - 1; i >= 0; i--) {                                       /* :304-329 */
            Vertex_Vote obj;
            obj.index = correspondences[initial_pos + vote_record[i].index].index;
            if (vote_record[i].score > num_selected) break;
            obj.score = (vote_record[i].score <= 50) ? 5.0f : 1.0f;
            selected_idx.push_back(obj);
        }
    }
}

/* ---- laserMapping.cpp:836-1030 (mapping's own vote: 20 regions, (double)expf(-gap^2) < 0.95, selected iff count < 0.75f * m) on
 * caller-supplied correspondences (ll_map_vote_host): count / selected per correspondence, in the caller's order */
inline void map_vote_host(Context &c, const std::vector<Corre_Match> &correspondences, std::vector<int> &count, std::vector<unsigned char> &selected)
{
    const int n = (int)correspondences.size();
    std::vector<ll_point> src(n), tgt(n);
    for (int i = 0; i < n; ++i) {
        src[i] = {correspondences[i].src.x, correspondences[i].src.y, correspondences[i].src.z, correspondences[i].src.intensity};
        tgt[i] = {correspondences[i].tgt.x, correspondences[i].tgt.y, correspondences[i].tgt.z, correspondences[i].tgt.intensity};
    }
    count.assign((size_t)n, 0); selected.assign((size_t)n, 0);
    c.check(ll_map_vote_host(c.get(), src.data(), tgt.data(), n, count.data(), selected.data()));
}

/* ---- the per-frame body of laserOdometry.cpp:439-832, one outer iteration at a time.
 * slot_curr holds the current scan's features (after laserCloudHandler), the target is what set_last() stored
 * (laserCloudCornerLast / laserCloudSurfLast, :882-896).  q = para_q (x,y,z,w), t = para_t (:61-62). */
class OdometryFrame {
public:
    explicit OdometryFrame(Context &c) : c_(c) {}
    /* kdtreeCornerLast->setInputCloud / kdtreeSurfLast->setInputCloud (:895-896) from host clouds ... */
    void set_last(const std::vector<PointXYZI> &cornerLast, const std::vector<PointXYZI> &surfLast) {
        c_.check(ll_set_target(c_.get(), (const ll_point *)cornerLast.data(), (int)cornerLast.size(),
                               (const ll_point *)surfLast.data(), (int)surfLast.size()));
    }
    /* ... or device-to-device from the slot that was just registered (the pointer swap of :882-888) */
    void set_last_from_slot(int slot) { c_.check(ll_set_target_from_slot(c_.get(), slot)); }

    /* correspondence search (:491-620, :653-793) + vote when now_frame > 5 (:794-810) + residual blocks + one
     * Gauss-Newton iteration of the problem Ceres would be handed (:820-825).  Updates q, t in place. */
    void iterate(int slot_curr, double q[4], double t[3], bool vote, ll_pair_info *info = nullptr) {
        const double pose[7] = {q[0], q[1], q[2], q[3], t[0], t[1], t[2]};
        c_.check(ll_associate_batch(c_.get(), slot_curr, 1, pose));
        c_.check(ll_vote_batch(c_.get(), slot_curr, 1, vote ? 1 : 0));
        c_.check(ll_normal_equations_batch(c_.get(), slot_curr, 1, nullptr));
        c_.check(ll_gn_step_batch(c_.get(), slot_curr, 1));
        double out[7];
        c_.check(ll_download_pose(c_.get(), slot_curr, out));
        for (int k = 0; k < 4; ++k) q[k] = out[k];
        for (int k = 0; k < 3; ++k) t[k] = out[4 + k];
        if (info) c_.check(ll_get_pair_info(c_.get(), slot_curr, info));
    }
private:
    Context &c_;
};

/* ---- laserMapping's optimisation block (first stage) -------------------------------------------------
 * What laserMapping.cpp:1822-2095 does once per frame, with the names it uses: the clouds gathered from the cube map,
 * the scan's down-sized feature clouds, parameters[7] = (q_w_curr x,y,z,w, t_w_curr).  The cube bookkeeping around it
 * (:1584-1808, :2101-2165) stays in the caller. */
class MapOptimizer {
public:
    MapOptimizer(Context &c, int max_map_corner, int max_map_surf, int max_scan_corner, int max_scan_surf) {
        c.check(ll_map_create(c.get(), max_map_corner, max_map_surf, max_scan_corner, max_scan_surf, &m_));
    }
    ~MapOptimizer() { ll_map_destroy(m_); }
    MapOptimizer(const MapOptimizer &) = delete;
    MapOptimizer &operator=(const MapOptimizer &) = delete;
    /* kdtreeCornerFromMap->setInputCloud(laserCloudCornerFromMap); kdtreeSurfFromMap->setInputCloud(...) (:1826-1827) */
    void setInputClouds(const std::vector<PointXYZI> &laserCloudCornerFromMap, const std::vector<PointXYZI> &laserCloudSurfFromMap) {
        check(ll_map_set_map(m_, (const ll_point *)laserCloudCornerFromMap.data(), (int)laserCloudCornerFromMap.size(),
                             (const ll_point *)laserCloudSurfFromMap.data(), (int)laserCloudSurfFromMap.size()));
    }
    /* laserCloudCornerStack / laserCloudSurfStack (:1813-1821) */
    void setScan(const std::vector<PointXYZI> &laserCloudCornerStack, const std::vector<PointXYZI> &laserCloudSurfStack) {
        check(ll_map_set_scan(m_, (const ll_point *)laserCloudCornerStack.data(), (int)laserCloudCornerStack.size(),
                              (const ll_point *)laserCloudSurfStack.data(), (int)laserCloudSurfStack.size()));
    }
    /* the `if (laserCloudCornerFromMapNum > 10 && laserCloudSurfFromMapNum > 50)` block: iterCount 0..1, data association
     * + ceres::Solve each.  Returns false where the reference prints "time Map corner and surf num are not enough". */
    bool optimize(double parameters[7], int iterations = 2) {
        int ran = 0;
        check(ll_map_optimize(m_, parameters, iterations, nullptr, &ran));
        return ran != 0;
    }
    void counts(int &corner_num, int &surf_num) { check(ll_map_get_counts(m_, &corner_num, &surf_num)); }
    /* the graph-based vote on the plane blocks (ll_map_set_vote; laserMapping.cpp:836-1030, :2057-2072): the data association then
     * keeps the selected blocks only, in stack order.  Off by default */
    void set_vote(bool on) { check(ll_map_set_vote(m_, on ? 1 : 0)); }
    /* the candidates of the last voted association, in stack order: stack index, incompatible pairs, selected flag, tgt (3 floats each) */
    void download_vote(std::vector<int> &src, std::vector<int> &count, std::vector<unsigned char> &selected, std::vector<float> &tgt3) {
        int n = 0;
        size_t cap = 1024;
        for (;;) {
            src.assign(cap, 0); count.assign(cap, 0); selected.assign(cap, 0); tgt3.assign(cap * 3, 0.0f);
            const int rc = ll_map_download_vote(m_, src.data(), count.data(), selected.data(), tgt3.data(), (int)cap, &n);
            if (rc == LL_ERR_CAPACITY && cap < ((size_t)1 << 24)) { cap *= 4; continue; }
            check(rc);
            break;
        }
        src.resize((size_t)n); count.resize((size_t)n); selected.resize((size_t)n); tgt3.resize((size_t)n * 3);
    }
    ll_map *get() const { return m_; }
private:
    void check(int rc) { if (rc != LL_OK) throw Error(rc, ll_map_last_error(m_)); }
    ll_map *m_ = nullptr;
};

/* ---- laserMapping's per-frame body with the cube map on the device (second stage) ---------------------
 * process() of laserMapping.cpp between transformAssociateToMap (:1581) and transformUpdate (:2101) plus the map update
 * (:2103-2165): the 21 x 21 x 11 cube arrays, their shifting, laserCloudCornerFromMap / SurfFromMap, the down-sized
 * scan, the optimisation, adding the registered scan and down-sizing the touched cubes.  What is left to the node: the
 * message queues, the two transform helpers below, publishing. */
class LaserMapping {
public:
    LaserMapping(Context &c, float lineRes = 0.4f, float planeRes = 0.8f, int max_scan_corner = 20000, int max_scan_surf = 200000,
                 int pool_points = 1 << 22) {
        c.check(ll_cubemap_create(c.get(), lineRes, planeRes, max_scan_corner, max_scan_surf, pool_points, &cm_));
    }
    ~LaserMapping() { ll_cubemap_destroy(cm_); }
    LaserMapping(const LaserMapping &) = delete;
    LaserMapping &operator=(const LaserMapping &) = delete;

    /* transformAssociateToMap (:113-117): q_w_curr = q_wmap_wodom * q_wodom_curr, t_w_curr = q_wmap_wodom * t_wodom_curr + t_wmap_wodom */
    void transformAssociateToMap(const double q_wodom_curr[4], const double t_wodom_curr[3]) {
        qmul(q_wmap_wodom, q_wodom_curr, parameters);
        double r[3]; qrot(q_wmap_wodom, t_wodom_curr, r);
        for (int k = 0; k < 3; ++k) parameters[4 + k] = r[k] + t_wmap_wodom[k];
    }
    /* transformUpdate (:119-123): q_wmap_wodom = q_w_curr * q_wodom_curr^-1, t_wmap_wodom = t_w_curr - q_wmap_wodom * t_wodom_curr */
    void transformUpdate(const double q_wodom_curr[4], const double t_wodom_curr[3]) {
        const double n2 = q_wodom_curr[0] * q_wodom_curr[0] + q_wodom_curr[1] * q_wodom_curr[1] + q_wodom_curr[2] * q_wodom_curr[2] + q_wodom_curr[3] * q_wodom_curr[3];
        const double inv[4] = {-q_wodom_curr[0] / n2, -q_wodom_curr[1] / n2, -q_wodom_curr[2] / n2, q_wodom_curr[3] / n2};
        qmul(parameters, inv, q_wmap_wodom);
        double r[3]; qrot(q_wmap_wodom, t_wodom_curr, r);
        for (int k = 0; k < 3; ++k) t_wmap_wodom[k] = parameters[4 + k] - r[k];
    }
    /* :1584-2165 for one frame; parameters[] holds the guess on entry and the optimised q_w_curr, t_w_curr on return */
    bool process(const std::vector<PointXYZI> &laserCloudCornerLast, const std::vector<PointXYZI> &laserCloudSurfLast) {
        int ran = 0;
        check(ll_cubemap_process(cm_, parameters, (const ll_point *)laserCloudCornerLast.data(), (int)laserCloudCornerLast.size(),
                                 (const ll_point *)laserCloudSurfLast.data(), (int)laserCloudSurfLast.size(), &ran));
        return ran != 0;
    }
    /* the same for the scan in an extracted slot of the context: nothing crosses the PCIe bus */
    bool process_slot(int slot) {
        int ran = 0;
        check(ll_cubemap_process_slot(cm_, parameters, slot, &ran));
        return ran != 0;
    }
    /* ---- tile-parallel over the GPUs of a node: one LaserMapping per rank, each keeping the cubes it
     * owns.  all_gather(send, recv, bytes): `bytes` from every rank into recv, rank-major (ncclAllGather / MPI_Allgather;
     * the buffers handed over are host memory).  Every rank passes the same scan and ends with the same parameters[]. */
    void set_shard(int rank, int world) { check(ll_cubemap_set_shard(cm_, rank, world)); world_ = world; }
    /* vote the plane blocks in process / process_slot (ll_cubemap_set_vote); not together with a shard */
    void set_vote(bool on) { check(ll_cubemap_set_vote(cm_, on ? 1 : 0)); }
    /* Failure discipline: nothing here throws between two collectives.  A rank whose library call failed remembers it, skips its
     * remaining library calls of the frame but still takes part in every all_gather of the sequence; the ranks exchange a status
     * word with the counts and once per outer iteration, so that ALL of them leave the frame at the same point -- each with an
     * exception (its own error, or "a peer failed") -- instead of one leaving and the others waiting in a gather for ever. */
    template <class AllGather>
    bool process_tile_parallel(const std::vector<PointXYZI> &laserCloudCornerLast, const std::vector<PointXYZI> &laserCloudSurfLast,
                               AllGather &&all_gather, const ll_lm_options *opt = nullptr) {
        std::string local_err; int local_rc = LL_OK;                                      /* first failure on this rank: message + its code */
        /* the message is fetched AFTER the call: as a second argument of step() it would be evaluated in an unspecified order (GCC:
         * right to left, i.e. before the failing call has assigned the error string it points into) */
        auto step = [&](int rc, auto last_err) { if (rc != LL_OK && local_err.empty()) { local_rc = rc; local_err = std::string(last_err()); } return rc == LL_OK; };
        auto cm_err = [&]() { return ll_cubemap_last_error(cm_); };
        auto any_failed = [&]() {                                                         /* one int per rank: a collective of its own */
            int mine = local_err.empty() ? 0 : 1;
            std::vector<int> all((size_t)world_);
            all_gather(&mine, all.data(), sizeof(int));
            for (int v : all) if (v) return true;
            return false;
        };
        auto leave = [&]() { if (local_err.empty()) throw Error(LL_ERR_STATE, std::string("process_tile_parallel: another rank failed")); throw Error(local_rc, local_err); };
        int cnt[4] = {0, 0, 0, 0};
        if (step(ll_cubemap_prepare(cm_, parameters + 4, (const ll_point *)laserCloudCornerLast.data(), (int)laserCloudCornerLast.size(),
                                    (const ll_point *)laserCloudSurfLast.data(), (int)laserCloudSurfLast.size()), cm_err))
            step(ll_cubemap_info(cm_, nullptr, cnt), cm_err);
        int mine[3] = {cnt[0], cnt[1], local_err.empty() ? 0 : 1};
        std::vector<int> all_cnt((size_t)3 * world_);
        all_gather(mine, all_cnt.data(), 3 * sizeof(int));
        long tot[2] = {0, 0}; bool failed = false;
        for (int r = 0; r < world_; ++r) { tot[0] += all_cnt[3 * r]; tot[1] += all_cnt[3 * r + 1]; failed = failed || all_cnt[3 * r + 2] != 0; }
        if (failed) leave();
        const bool ran = tot[0] > 10 && tot[1] > 50;                                      /* :1822 */
        if (ran) {
            ll_map *m = ll_cubemap_map(cm_);
            auto m_err = [&]() { return ll_map_last_error(m); };
            const size_t nc = (size_t)cnt[2] * 5, ns = (size_t)cnt[3] * 5;
            /* ONE all_gather per outer iteration: a rank's status word and its four candidate arrays travel as one packed record
             * [status | corner (x, y, z, d) | corner ids | surf (x, y, z, d) | surf ids] (every rank holds the whole scan, so the
             * records have one size); the receiver lays the parts out rank-major again for ll_map_associate_merged.  (Four gathers
             * and a status gather per iteration were five host-staged collectives, each with its own stream synchronisation.) */
            const size_t o_cn = 4, o_ci = o_cn + nc * 16, o_sn = o_ci + nc * 4, o_si = o_sn + ns * 16, rec = o_si + ns * 4;
            std::vector<unsigned char> pack(rec), all(rec * (size_t)world_);
            std::vector<float> acn(nc * 4 * world_ + 4), asn(ns * 4 * world_ + 4);
            std::vector<int> aci(nc * world_ + 1), asi(ns * world_ + 1);
            for (int it = 0; it < 2; ++it) {                                              /* :1832 */
                if (local_err.empty())
                    step(ll_map_knn_partial(m, parameters, (float *)(pack.data() + o_cn), (int *)(pack.data() + o_ci),
                                            (float *)(pack.data() + o_sn), (int *)(pack.data() + o_si)), m_err);
                const int mine_st = local_err.empty() ? 0 : 1;
                std::memcpy(pack.data(), &mine_st, sizeof(int));
                all_gather(pack.data(), all.data(), rec);
                bool bad = false;
                for (int r = 0; r < world_; ++r) {
                    const unsigned char *q = all.data() + (size_t)r * rec;
                    int st; std::memcpy(&st, q, sizeof(int)); bad = bad || st != 0;
                    std::memcpy((unsigned char *)acn.data() + (size_t)r * nc * 16, q + o_cn, nc * 16);
                    std::memcpy((unsigned char *)aci.data() + (size_t)r * nc * 4, q + o_ci, nc * 4);
                    std::memcpy((unsigned char *)asn.data() + (size_t)r * ns * 16, q + o_sn, ns * 16);
                    std::memcpy((unsigned char *)asi.data() + (size_t)r * ns * 4, q + o_si, ns * 4);
                }
                if (bad) leave();                                                         /* every rank takes this exit in the same iteration */
                if (step(ll_map_associate_merged(m, parameters, world_, acn.data(), aci.data(), asn.data(), asi.data()), m_err))
                    step(ll_map_solve(m, parameters, opt), m_err);
            }
            if (any_failed()) leave();                                                    /* the last iteration's merge / solve */
        }
        check(ll_cubemap_update(cm_, parameters));                                        /* local to the rank: no collective behind it in this frame */
        return ran;
    }
    /* laserCloudSurround (LL_MAP_SURROUND, :2173-2181: the cubes of the last frame's laserCloudSurroundInd) or laserCloudMap
     * (LL_MAP_ALL, :2190-2197: all 4851 cubes), per cube the corner cloud then the surf cloud: one gather, one copy */
    void export_map(int which, std::vector<PointXYZI> &out) {
        long long n = 0;
        ll_point none;
        const int rc = ll_cubemap_export(cm_, which, &none, 0, &n);                       /* the size: with points to write nothing is launched */
        if (rc != LL_ERR_CAPACITY) check(rc);
        out.resize((size_t)n);
        if (n > 0) check(ll_cubemap_export(cm_, which, (ll_point *)out.data(), n, &n));
    }
    double parameters[7] = {0, 0, 0, 1, 0, 0, 0};                 /* :81-83 */
    double q_wmap_wodom[4] = {0, 0, 0, 1}, t_wmap_wodom[3] = {0, 0, 0};   /* :88-89 */
    ll_cubemap *get() const { return cm_; }
private:
    static void qmul(const double a[4], const double b[4], double o[4]) {
        const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
        o[0] = aw * bx + ax * bw + ay * bz - az * by; o[1] = aw * by - ax * bz + ay * bw + az * bx;
        o[2] = aw * bz + ax * by - ay * bx + az * bw; o[3] = aw * bw - ax * bx - ay * by - az * bz;
    }
    static void qrot(const double q[4], const double v[3], double o[3]) {
        const double ux = q[0], uy = q[1], uz = q[2], w = q[3];
        double uvx = uy * v[2] - uz * v[1], uvy = uz * v[0] - ux * v[2], uvz = ux * v[1] - uy * v[0];
        uvx += uvx; uvy += uvy; uvz += uvz;
        o[0] = v[0] + w * uvx + (uy * uvz - uz * uvy); o[1] = v[1] + w * uvy + (uz * uvx - ux * uvz); o[2] = v[2] + w * uvz + (ux * uvy - uy * uvx);
    }
    void check(int rc) { if (rc != LL_OK) throw Error(rc, ll_cubemap_last_error(cm_)); }
    static void mcheck(ll_map *m, int rc) { if (rc != LL_OK) throw Error(rc, ll_map_last_error(m)); }
    ll_cubemap *cm_ = nullptr;
    int world_ = 1;
    friend class LaserMappingSequences;
};

/* ll_cubemaps_layout of one map: the centre, the per-cube point counts [2][4851] (corner, then surf) and the valid list of its
 * last frame */
/* Keyframes (ll_keyframes): the stack clouds (down-sized corner and surf features, sensor frame) and mapped poses of frames, kept on
 * the device; ids are 0 .. size() - 1 in the order of the adds.  LaserMappingSequences::insert_keyframes rebuilds cube maps from them
 * under corrected poses.  Destroy it before its Context, and after every Drives that captures into it. */
class Keyframes {
public:
    struct Exported { std::vector<PointXYZI> points; std::vector<long long> offsets; };   /* cloud w of frame first + f: points[offsets[2 f + w] .. offsets[2 f + w + 1]) */
    Keyframes(Context &c, int max_frames, long long cap_corner, long long cap_surf) {
        ll_keyframes_params p;
        p.max_frames = max_frames; p.cap_corner = cap_corner; p.cap_surf = cap_surf;
        c.check(ll_keyframes_create(c.get(), &p, &kf_));
    }
    ~Keyframes() { ll_keyframes_destroy(kf_); }
    Keyframes(const Keyframes &) = delete;
    Keyframes &operator=(const Keyframes &) = delete;

    int size() const { return ll_keyframes_size(kf_); }
    void reset() { check(ll_keyframes_reset(kf_)); }
    ll_keyframe_info info(int id) const {
        ll_keyframe_info e;
        check(ll_keyframes_info(kf_, id, &e));
        return e;
    }
    /* one keyframe per sequence with sel[q] != 0 from the stack clouds of its last frame and pose_w7 [S][7]: one copy launch, no
     * synchronisation; the first new id (-1: none selected).  cms: LaserMappingSequences::get() or Drives::cubemaps() */
    int add_cubemaps(ll_cubemaps *cms, const std::vector<int> &sel, const double *pose_w7, const int *lane_tag = nullptr, const int *frame_tag = nullptr) {
        int first = -1;
        check(ll_keyframes_add_cubemaps(kf_, cms, sel.data(), pose_w7, lane_tag, frame_tag, &first));
        return first;
    }
    int add_points(const std::vector<PointXYZI> &corner, const std::vector<PointXYZI> &surf, const double *pose_w7) {
        int id = -1;
        check(ll_keyframes_add_points(kf_, (const ll_point *)corner.data(), (int)corner.size(), (const ll_point *)surf.data(), (int)surf.size(), pose_w7, &id));
        return id;
    }
    /* frames first .. first + count - 1 back to back, per frame the corner cloud, then the surf cloud: one gather, one copy, one synchronisation */
    Exported export_frames(int first, int count) {
        Exported x;
        x.offsets.assign((size_t)2 * (count > 0 ? count : 0) + 1, 0);
        check(ll_keyframes_export(kf_, first, count, nullptr, x.offsets.data()));
        x.points.resize((size_t)x.offsets.back());
        if (!x.points.empty()) check(ll_keyframes_export(kf_, first, count, (ll_point *)x.points.data(), x.offsets.data()));
        return x;
    }
    ll_keyframes *get() const { return kf_; }
private:
    void check(int rc) const { if (rc != LL_OK) throw Error(rc, ll_keyframes_last_error(kf_)); }
    ll_keyframes *kf_ = nullptr;
};

/* Visibility (ll_visibility): per point of a Keyframes store how many other frames of its drive saw through it and how many hit it;
 * LaserMappingSequences::insert_keyframes_filtered leaves the points out that a rule over the two counters removes.  Destroy it
 * before its store. */
class Visibility {
public:
    struct Counts { std::vector<unsigned char> corner, surf; };   /* [n][2]: through, hit */
    static ll_visibility_params default_params() { ll_visibility_params p; ll_visibility_default_params(&p); return p; }
    explicit Visibility(Keyframes &kf) : Visibility(kf, default_params()) {}
    Visibility(Keyframes &kf, const ll_visibility_params &p) : kf_(&kf), p_(p) {
        const int rc = ll_visibility_create(kf.get(), &p, &v_);
        if (rc != LL_OK) throw Error(rc, ll_keyframes_last_error(kf.get()));
    }
    ~Visibility() { ll_visibility_destroy(v_); }
    Visibility(const Visibility &) = delete;
    Visibility &operator=(const Visibility &) = delete;

    /* every op is one drive whose listed frames observe each other; the ordered frame pairs per op */
    std::vector<long long> run(const std::vector<ll_visibility_op> &ops) {
        std::vector<long long> pairs(ops.size(), 0);
        check(ll_visibility_run(v_, ops.data(), (int)ops.size(), pairs.data()));
        return pairs;
    }
    Counts counts(int frame) {
        const ll_keyframe_info e = kf_->info(frame);
        std::vector<unsigned char> all((size_t)2 * (e.n[0] + e.n[1]) + 1, 0);
        check(ll_visibility_counts(v_, frame, all.data()));
        Counts c;
        c.corner.assign(all.begin(), all.begin() + (size_t)2 * e.n[0]);
        c.surf.assign(all.begin() + (size_t)2 * e.n[0], all.begin() + (size_t)2 * (e.n[0] + e.n[1]));
        return c;
    }
    /* raw / img [height][width] of the k-th listed frame of the last run */
    void images(int k, std::vector<float> *raw, std::vector<float> *img) {
        const size_t n = (size_t)p_.width * p_.height;
        if (raw) raw->assign(n, 0.0f);
        if (img) img->assign(n, 0.0f);
        check(ll_visibility_images(v_, k, raw ? raw->data() : nullptr, img ? img->data() : nullptr));
    }
    void reset() { check(ll_visibility_reset(v_)); }
    void timing(double ms[3], long long counts[3]) const { check(ll_visibility_timing(v_, ms, counts)); }
    const ll_visibility_params &params() const { return p_; }
    ll_visibility *get() const { return v_; }
private:
    void check(int rc) const { if (rc != LL_OK) throw Error(rc, ll_visibility_last_error(v_)); }
    Keyframes *kf_;
    ll_visibility_params p_;
    ll_visibility *v_ = nullptr;
};

/* Bev (ll_bev): correlative matching of bird's-eye occupancy grids over a Keyframes store -- from a place match (the revisited frame,
 * a heading good to a sector) to the 3-DoF transform D that starts an align (guess) or a localising lane.  Destroy it before its
 * store. */
class Bev {
public:
    static ll_bev_params default_params() { ll_bev_params p; ll_bev_default_params(&p); return p; }
    explicit Bev(Keyframes &kf) : Bev(kf, default_params()) {}
    Bev(Keyframes &kf, const ll_bev_params &p) : p_(p) {
        const int rc = ll_bev_create(kf.get(), &p, &b_);
        if (rc != LL_OK) throw Error(rc, ll_keyframes_last_error(kf.get()));
    }
    ~Bev() { ll_bev_destroy(b_); }
    Bev(const Bev &) = delete;
    Bev &operator=(const Bev &) = delete;

    /* one result per op; one upload, one fill, three launches, one synchronisation whatever ops.size() is */
    std::vector<ll_bev_result> match(const std::vector<ll_bev_op> &ops) {
        std::vector<ll_bev_result> out(ops.size());
        check(ll_bev_match(b_, ops.data(), (int)ops.size(), out.data()));
        n_yaws_.resize(ops.size());
        for (size_t i = 0; i < ops.size(); ++i) n_yaws_[i] = ops[i].n_yaws;
        return out;
    }
    /* the scores [n_yaws][2 sh][2 sh] of op `op` of the last match */
    std::vector<int> volume(int op) {
        const size_t n = op >= 0 && (size_t)op < n_yaws_.size() ? (size_t)n_yaws_[op] : 1;
        std::vector<int> v(n * 4 * p_.shift_half * p_.shift_half, 0);
        check(ll_bev_volume(b_, op, v.data()));
        return v;
    }
    /* the target grid [2 half][2 half] of op `op` of the last match */
    std::vector<unsigned char> grid(int op) {
        std::vector<unsigned char> g((size_t)4 * p_.half * p_.half, 0);
        check(ll_bev_grid(b_, op, g.data()));
        return g;
    }
    void reset() { check(ll_bev_reset(b_)); n_yaws_.clear(); }
    void timing(double ms[3], long long counts[3]) const { check(ll_bev_timing(b_, ms, counts)); }
    /* T0 = P_c o D o P_q^-1: the guess of an align of the query's map onto the candidate's */
    static void guess(const double Pc_w7[7], const double D_w7[7], const double Pq_w7[7], double T0_w7[7]) {
        const int rc = ll_bev_guess(Pc_w7, D_w7, Pq_w7, T0_w7);
        if (rc != LL_OK) throw Error(rc, "bev guess: a NULL pointer");
    }
    const ll_bev_params &params() const { return p_; }
    ll_bev *get() const { return b_; }
private:
    void check(int rc) const { if (rc != LL_OK) throw Error(rc, ll_bev_last_error(b_)); }
    ll_bev_params p_;
    ll_bev *b_ = nullptr;
    std::vector<int> n_yaws_;
};

/* Entropy (ll_entropy): mean map entropy and mean plane variance of the cloud that listed frames of a Keyframes store make under
 * listed poses -- the same frames before and after a pose-graph solve in one call.  It rewards any thinning: compare trajectories
 * over the same points only.  Destroy it before its store. */
class Entropy {
public:
    struct Values { std::vector<float> h, pv; std::vector<unsigned short> nn; };   /* [n_corner + n_surf], corner first */
    static ll_entropy_params default_params() { ll_entropy_params p; ll_entropy_default_params(&p); return p; }
    explicit Entropy(Keyframes &kf) : Entropy(kf, default_params()) {}
    Entropy(Keyframes &kf, const ll_entropy_params &p) : kf_(&kf), p_(p) {
        const int rc = ll_entropy_create(kf.get(), &p, &e_);
        if (rc != LL_OK) throw Error(rc, ll_keyframes_last_error(kf.get()));
    }
    ~Entropy() { ll_entropy_destroy(e_); }
    Entropy(const Entropy &) = delete;
    Entropy &operator=(const Entropy &) = delete;

    /* one record per op; two synchronisations (and the sort's read-back above 65536 points) whatever ops.size() is */
    std::vector<ll_entropy_rec> run(const std::vector<ll_entropy_op> &ops) {
        std::vector<ll_entropy_rec> rec(ops.size());
        check(ll_entropy_run(e_, ops.data(), (int)ops.size(), rec.data()));
        sizes_.clear();
        for (size_t i = 0; i < ops.size(); ++i)
            for (int f = 0; f < ops[i].n_frames; ++f) {
                const ll_keyframe_info e = kf_->info(ops[i].frames[f]);
                sizes_.push_back((size_t)e.n[0] + (size_t)e.n[1]);
            }
        return rec;
    }
    /* the k-th listed frame, counted across ops, of the last run */
    Values values(int k) {
        const size_t n = k >= 0 && (size_t)k < sizes_.size() ? sizes_[k] : 0;
        Values v;
        v.h.assign(n + 1, 0.0f); v.pv.assign(n + 1, 0.0f); v.nn.assign(n + 1, 0);
        check(ll_entropy_values(e_, k, v.h.data(), v.pv.data(), v.nn.data()));
        v.h.resize(n); v.pv.resize(n); v.nn.resize(n);
        return v;
    }
    void reset() { check(ll_entropy_reset(e_)); sizes_.clear(); }
    void timing(double ms[5], long long counts[5]) const { check(ll_entropy_timing(e_, ms, counts)); }
    const ll_entropy_params &params() const { return p_; }
    ll_entropy *get() const { return e_; }
private:
    void check(int rc) const { if (rc != LL_OK) throw Error(rc, ll_entropy_last_error(e_)); }
    Keyframes *kf_;
    ll_entropy_params p_;
    ll_entropy *e_ = nullptr;
    std::vector<size_t> sizes_;
};

struct MapLayout {
    enum { N_COUNTS = 2 * 4851 };
    int cen[3] = {10, 10, 5};
    std::vector<int> counts = std::vector<int>((size_t)N_COUNTS, 0), valid = std::vector<int>(125, 0);
};

/* laserMapping for S sequences side by side (ll_cubemaps): per sequence q the state of LaserMapping (parameters, q_wmap_wodom,
 * t_wmap_wodom, rows of [S][7] / [S][4] / [S][3]) and the same formulas; one call runs frame k of every running sequence.
 * Sequence q equals a LaserMapping fed the same frames, bit for bit. */
class LaserMappingSequences {
public:
    LaserMappingSequences(Context &c, int n_seq, float lineRes = 0.4f, float planeRes = 0.8f, int max_scan_corner = 20000,
                          int max_scan_surf = 200000, int pool_points = 1 << 22)
        : S(n_seq), parameters((size_t)7 * n_seq), q_wmap_wodom((size_t)4 * n_seq), t_wmap_wodom((size_t)3 * n_seq, 0.0), ran((size_t)n_seq, 0) {
        c.check(ll_cubemaps_create(c.get(), n_seq, lineRes, planeRes, max_scan_corner, max_scan_surf, pool_points, &cms_));
        for (int q = 0; q < S; ++q) {
            const double p0[7] = {0, 0, 0, 1, 0, 0, 0}, q0[4] = {0, 0, 0, 1};
            std::copy(p0, p0 + 7, &parameters[(size_t)7 * q]); std::copy(q0, q0 + 4, &q_wmap_wodom[(size_t)4 * q]);
        }
    }
    ~LaserMappingSequences() { ll_cubemaps_destroy(cms_); }
    LaserMappingSequences(const LaserMappingSequences &) = delete;
    LaserMappingSequences &operator=(const LaserMappingSequences &) = delete;

    /* transformAssociateToMap / transformUpdate (:113-123) of every sequence q with run[q] (NULL: all); q_wodom_curr [S][4], t [S][3] */
    void transformAssociateToMap(const double *q_wodom_curr, const double *t_wodom_curr, const int *run = nullptr) {
        for (int q = 0; q < S; ++q) {
            if (run && !run[q]) continue;
            double *P = &parameters[(size_t)7 * q];
            const double *qm = &q_wmap_wodom[(size_t)4 * q], *tm = &t_wmap_wodom[(size_t)3 * q];
            LaserMapping::qmul(qm, q_wodom_curr + 4 * q, P);
            double r[3]; LaserMapping::qrot(qm, t_wodom_curr + 3 * q, r);
            for (int k = 0; k < 3; ++k) P[4 + k] = r[k] + tm[k];
        }
    }
    void transformUpdate(const double *q_wodom_curr, const double *t_wodom_curr, const int *run = nullptr) {
        for (int q = 0; q < S; ++q) {
            if (run && !run[q]) continue;
            const double *qc = q_wodom_curr + 4 * q, *P = &parameters[(size_t)7 * q];
            double *qm = &q_wmap_wodom[(size_t)4 * q], *tm = &t_wmap_wodom[(size_t)3 * q];
            const double n2 = qc[0] * qc[0] + qc[1] * qc[1] + qc[2] * qc[2] + qc[3] * qc[3];
            const double inv[4] = {-qc[0] / n2, -qc[1] / n2, -qc[2] / n2, qc[3] / n2};
            LaserMapping::qmul(P, inv, qm);
            double r[3]; LaserMapping::qrot(qm, t_wodom_curr + 3 * q, r);
            for (int k = 0; k < 3; ++k) tm[k] = P[4 + k] - r[k];
        }
    }
    /* :1584-2165 for every sequence q with slots[q] >= 0 (its scan: that extracted slot of the context); parameters rows in: the
     * guesses, out: the optimised poses; ran[q] as LaserMapping::process_slot returns it */
    void process_slots(const std::vector<int> &slots) {
        if ((int)slots.size() != S) throw Error(LL_ERR_ARG, "one slot per sequence");
        check(ll_cubemaps_process_slots(cms_, slots.data(), parameters.data(), ran.data()));
    }
    /* on[q] != 0: sequence q votes its plane blocks in process_slots / process from now on (ll_cubemaps_set_vote); localize_slots never votes */
    void set_vote(const std::vector<int> &on) {
        if ((int)on.size() != S) throw Error(LL_ERR_ARG, "one flag per sequence");
        check(ll_cubemaps_set_vote(cms_, on.data()));
    }
    /* a READ-ONLY frame (ll_cubemaps_localize_slots): sequence q with slots[q] >= 0 localises that extracted slot against map
     * map_of[q] (an empty map_of: its own map) from the guess in its parameters row; no map changes, several sequences may read
     * one map.  parameters / ran as process_slots leaves them; with want_fit, fit[q] says how the pose fits the map (zeros for a
     * sequence that did not optimise; rows of sequences that sat out keep what they held) */
    void localize_slots(const std::vector<int> &slots, const std::vector<int> &map_of = std::vector<int>(), bool want_fit = true) {
        if ((int)slots.size() != S || (!map_of.empty() && (int)map_of.size() != S)) throw Error(LL_ERR_ARG, "one slot (and one map) per sequence");
        if (want_fit && fit.empty()) fit.assign((size_t)S, ll_localize_fit());
        check(ll_cubemaps_localize_slots(cms_, slots.data(), map_of.empty() ? nullptr : map_of.data(), parameters.data(), ran.data(),
                                         want_fit ? fit.data() : nullptr));
    }
    /* the same with the information of every solve at its final pose (ll_cubemaps_localize_slots_info): info [S], zeros for a sequence
     * that sat out or did not optimise.  PoseGraphs::edge_from_info turns a record and the row's pose into an edge's weight */
    void localize_slots(const std::vector<int> &slots, const std::vector<int> &map_of, bool want_fit, std::vector<PoseInfo> *info) {
        if ((int)slots.size() != S || (!map_of.empty() && (int)map_of.size() != S)) throw Error(LL_ERR_ARG, "one slot (and one map) per sequence");
        if (want_fit && fit.empty()) fit.assign((size_t)S, ll_localize_fit());
        if (info) info->assign((size_t)S, PoseInfo());
        check(ll_cubemaps_localize_slots_info(cms_, slots.data(), map_of.empty() ? nullptr : map_of.data(), parameters.data(), ran.data(),
                                              want_fit ? fit.data() : nullptr, info ? info->data() : nullptr));
    }
    /* the same from host clouds; an empty pair of clouds with run[q] == 0 (or both pointers NULL) skips sequence q */
    void process(const std::vector<const std::vector<PointXYZI> *> &corner_last, const std::vector<const std::vector<PointXYZI> *> &surf_last) {
        if ((int)corner_last.size() != S || (int)surf_last.size() != S) throw Error(LL_ERR_ARG, "one cloud pair per sequence");
        std::vector<const ll_point *> c((size_t)S, nullptr), s((size_t)S, nullptr);
        std::vector<int> nc((size_t)S, 0), ns((size_t)S, 0);
        static const ll_point empty = {0, 0, 0, 0};
        for (int q = 0; q < S; ++q) {
            if (!corner_last[q] && !surf_last[q]) continue;
            c[q] = corner_last[q] && !corner_last[q]->empty() ? (const ll_point *)corner_last[q]->data() : &empty;
            s[q] = surf_last[q] && !surf_last[q]->empty() ? (const ll_point *)surf_last[q]->data() : &empty;
            nc[q] = corner_last[q] ? (int)corner_last[q]->size() : 0; ns[q] = surf_last[q] ? (int)surf_last[q]->size() : 0;
        }
        check(ll_cubemaps_process(cms_, c.data(), nc.data(), s.data(), ns.data(), parameters.data(), ran.data()));
    }
    /* the map publications (:2173-2203) of the sequences which[q] selects (LL_MAP_NONE / LL_MAP_SURROUND / LL_MAP_ALL), back to
     * back in sequence order: sequence q is out[offset[q] .. offset[q + 1]).  One gather, one copy, one synchronisation */
    void export_maps(const std::vector<int> &which, std::vector<PointXYZI> &out, std::vector<long long> &offset) {
        if ((int)which.size() != S) throw Error(LL_ERR_ARG, "one selection per sequence");
        const int rc = export_from(cms_, S, which.data(), out, offset);
        if (rc != LL_OK) check(rc);
    }
    /* what an LL_MAP_ALL export does not say about map q (ll_cubemaps_layout: host bookkeeping, no launch); with that cloud the
     * complete state of the map */
    MapLayout layout(int q) {
        MapLayout L;
        int n = 0;
        check(ll_cubemaps_layout(cms_, q, L.cen, L.counts.data(), L.valid.data(), &n));
        L.valid.resize((size_t)n);
        return L;
    }
    /* the export's inverse (ll_cubemaps_import): points / offset as export_maps(LL_MAP_ALL) gave them, layouts[q] == nullptr leaves
     * map q alone.  One upload, one scatter, one synchronisation */
    void import_maps(const std::vector<PointXYZI> &points, const std::vector<long long> &offset, const std::vector<const MapLayout *> &layouts) {
        if ((int)layouts.size() != S || (int)offset.size() != S + 1) throw Error(LL_ERR_ARG, "one layout per sequence and S + 1 offsets");
        if (offset[(size_t)S] > (long long)points.size()) throw Error(LL_ERR_ARG, "points is shorter than offset[S]");
        const int rc = import_into(cms_, S, points.data(), offset.data(), layouts);
        if (rc != LL_OK) check(rc);
    }
    /* ll_cubemaps_merge: op i takes map ops[i].src through pointAssociateToMap with ops[i].T_w7 into map ops[i].dst and filters every
     * cube that received a point.  added / dropped [n_ops][2] (corner, surf) when given.  Everything on the device */
    void merge_maps(const std::vector<ll_merge_op> &ops, std::vector<long long> *added = nullptr, std::vector<long long> *dropped = nullptr) {
        const int rc = merge_into(cms_, ops, added, dropped);
        if (rc != LL_OK) check(rc);
    }
    /* the same on a borrowed handle (Drives::cubemaps(), between two steps); returns the status */
    static int merge_into(ll_cubemaps *cms, const std::vector<ll_merge_op> &ops, std::vector<long long> *added = nullptr, std::vector<long long> *dropped = nullptr) {
        if (added) added->assign(2 * ops.size(), 0);
        if (dropped) dropped->assign(2 * ops.size(), 0);
        return ll_cubemaps_merge(cms, ops.data(), (int)ops.size(), added ? added->data() : nullptr, dropped ? dropped->data() : nullptr);
    }
    /* ll_cubemaps_insert_keyframes: op i places the listed frames of the store into map ops[i].dst, each frame under its own pose
     * (ops[i].poses_w7, or the stored poses when NULL), after emptying dst when ops[i].reset is set; every cube that received a point is
     * filtered ONCE over its old cloud and all new points (the merge's semantics, not frame-by-frame mapping).  added / dropped
     * [n_ops][2] (corner, surf) when given.  Everything on the device */
    void insert_keyframes(const Keyframes &kf, const std::vector<ll_insert_op> &ops, std::vector<long long> *added = nullptr, std::vector<long long> *dropped = nullptr) {
        const int rc = insert_into(cms_, kf, ops, added, dropped);
        if (rc != LL_OK) check(rc);
    }
    /* the same on a borrowed handle (Drives::cubemaps(), between two steps); returns the status */
    static int insert_into(ll_cubemaps *cms, const Keyframes &kf, const std::vector<ll_insert_op> &ops, std::vector<long long> *added = nullptr, std::vector<long long> *dropped = nullptr) {
        if (added) added->assign(2 * ops.size(), 0);
        if (dropped) dropped->assign(2 * ops.size(), 0);
        return ll_cubemaps_insert_keyframes(cms, kf.get(), ops.data(), (int)ops.size(), added ? added->data() : nullptr, dropped ? dropped->data() : nullptr);
    }
    /* ll_cubemaps_insert_keyframes_filtered: the same with the points left out that `rule` removes by vis's counters (through >=
     * min_through && hit <= max_hit); removed [n_ops][2] when given; added + dropped + removed = the listed points */
    void insert_keyframes_filtered(const Keyframes &kf, const Visibility &vis, const ll_visibility_rule &rule, const std::vector<ll_insert_op> &ops,
                                   std::vector<long long> *added = nullptr, std::vector<long long> *dropped = nullptr, std::vector<long long> *removed = nullptr) {
        const int rc = insert_filtered_into(cms_, kf, vis, rule, ops, added, dropped, removed);
        if (rc != LL_OK) check(rc);
    }
    static int insert_filtered_into(ll_cubemaps *cms, const Keyframes &kf, const Visibility &vis, const ll_visibility_rule &rule, const std::vector<ll_insert_op> &ops,
                                    std::vector<long long> *added = nullptr, std::vector<long long> *dropped = nullptr, std::vector<long long> *removed = nullptr) {
        if (added) added->assign(2 * ops.size(), 0);
        if (dropped) dropped->assign(2 * ops.size(), 0);
        if (removed) removed->assign(2 * ops.size(), 0);
        return ll_cubemaps_insert_keyframes_filtered(cms, kf.get(), vis.get(), &rule, ops.data(), (int)ops.size(), added ? added->data() : nullptr,
                                                     dropped ? dropped->data() : nullptr, removed ? removed->data() : nullptr);
    }
    /* ll_cubemaps_align: op i estimates the transform that takes map ops[i].src's world frame into map ops[i].dst's, starting at
     * ops[i].T_w7 -- laserMapping's optimisation over the whole of both maps, read-only.  T [n_ops][7]; ran [n_ops] and fit [n_ops]
     * when given (fit == nullptr: the extra pass at the final poses is not launched).  Follow it with merge_maps under T */
    void align_maps(const std::vector<ll_merge_op> &ops, int n_outer, std::vector<double> *T, std::vector<int> *ran = nullptr,
                    std::vector<ll_localize_fit> *fit = nullptr, const ll_lm_options *opt = nullptr) {
        const int rc = align_into(cms_, ops, n_outer, T, ran, fit, opt);
        if (rc != LL_OK) check(rc);
    }
    /* the same with the information of every op at its final T (ll_cubemaps_align_info): info [n_ops] */
    void align_maps(const std::vector<ll_merge_op> &ops, int n_outer, std::vector<double> *T, std::vector<int> *ran,
                    std::vector<ll_localize_fit> *fit, std::vector<PoseInfo> *info, const ll_lm_options *opt = nullptr) {
        if (!T) check(LL_ERR_ARG);
        T->assign(7 * ops.size(), 0.0);
        if (ran) ran->assign(ops.size(), 0);
        if (fit) fit->assign(ops.size(), ll_localize_fit());
        if (info) info->assign(ops.size(), PoseInfo());
        check(ll_cubemaps_align_info(cms_, ops.data(), (int)ops.size(), n_outer, opt, T->data(), ran ? ran->data() : nullptr,
                                     fit ? fit->data() : nullptr, info ? info->data() : nullptr));
    }
    /* the same on a borrowed handle (Drives::cubemaps(), between two steps); returns the status */
    static int align_into(ll_cubemaps *cms, const std::vector<ll_merge_op> &ops, int n_outer, std::vector<double> *T, std::vector<int> *ran = nullptr,
                          std::vector<ll_localize_fit> *fit = nullptr, const ll_lm_options *opt = nullptr) {
        if (!T) return LL_ERR_ARG;
        T->assign(7 * ops.size(), 0.0);
        if (ran) ran->assign(ops.size(), 0);
        if (fit) fit->assign(ops.size(), ll_localize_fit());
        return ll_cubemaps_align(cms, ops.data(), (int)ops.size(), n_outer, opt, T->data(), ran ? ran->data() : nullptr, fit ? fit->data() : nullptr);
    }
    static int import_into(ll_cubemaps *cms, int n_seq, const PointXYZI *points, const long long *offset, const std::vector<const MapLayout *> &layouts) {
        const size_t S_ = (size_t)n_seq;
        std::vector<int> sel(S_, 0), cen(3 * S_, 0), counts(S_ * MapLayout::N_COUNTS, 0), valid(S_ * 125, 0), nv(S_, 0);
        for (size_t q = 0; q < S_; ++q) {
            const MapLayout *L = layouts[q];
            if (!L) continue;
            if (L->counts.size() != (size_t)MapLayout::N_COUNTS || L->valid.size() > 125) return LL_ERR_ARG;
            sel[q] = 1; nv[q] = (int)L->valid.size();
            std::copy(L->cen, L->cen + 3, &cen[3 * q]);
            std::copy(L->counts.begin(), L->counts.end(), &counts[q * MapLayout::N_COUNTS]);
            std::copy(L->valid.begin(), L->valid.end(), &valid[q * 125]);
        }
        return ll_cubemaps_import(cms, sel.data(), (const ll_point *)points, offset, cen.data(), counts.data(), valid.data(), nv.data());
    }
    /* the same on a borrowed handle (Drives::export_maps); returns the status, the text is the handle's last error */
    static int export_from(ll_cubemaps *cms, int n_seq, const int *which, std::vector<PointXYZI> &out, std::vector<long long> &offset) {
        offset.assign((size_t)n_seq + 1, 0);
        int rc = ll_cubemaps_export_sizes(cms, which, offset.data());
        if (rc != LL_OK) return rc;
        out.resize((size_t)offset[(size_t)n_seq]);
        return ll_cubemaps_export(cms, which, (ll_point *)out.data(), (long long)out.size(), offset.data());
    }
    const int S;
    std::vector<double> parameters, q_wmap_wodom, t_wmap_wodom;   /* [S][7], [S][4], [S][3] */
    std::vector<int> ran;                                       /* [S] */
    std::vector<ll_localize_fit> fit;                           /* [S] once localize_slots has asked for it */
    ll_cubemaps *get() const { return cms_; }
private:
    void check(int rc) { if (rc != LL_OK) throw Error(rc, ll_cubemaps_last_error(cms_)); }
    ll_cubemaps *cms_ = nullptr;
};

/* ---- I/O surface ---------------------------------------------------------------------------------- */

/* KITTI velodyne .bin: float32 (x, y, z, reflectance) per point -- src/kittiHelper.cpp:22-32, same name */
inline std::vector<float> read_lidar_data(const std::string &lidar_data_path)
{
    std::FILE *f = std::fopen(lidar_data_path.c_str(), "rb");
    if (!f) throw Error(LL_ERR_ARG, "cannot open " + lidar_data_path);
    std::fseek(f, 0, SEEK_END);
    const size_t num_elements = (size_t)std::ftell(f) / sizeof(float);
    std::fseek(f, 0, SEEK_SET);
    std::vector<float> lidar_data_buffer(num_elements);
    const size_t got = std::fread(lidar_data_buffer.data(), sizeof(float), num_elements, f);
    std::fclose(f);
    lidar_data_buffer.resize(got);
    return lidar_data_buffer;
}

/* World pose accumulation of laserOdometry (:830-831): t_w = t_w + q_w * t ; q_w = q_w * q   (q = x,y,z,w) */
struct WorldPose {
    double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
    void compose(const double ql[4], const double tl[3]) {
        const double ux = q[0], uy = q[1], uz = q[2], w = q[3];
        double uv[3] = {uy * tl[2] - uz * tl[1], uz * tl[0] - ux * tl[2], ux * tl[1] - uy * tl[0]};
        for (double &v : uv) v += v;
        t[0] += (tl[0] + w * uv[0]) + (uy * uv[2] - uz * uv[1]);
        t[1] += (tl[1] + w * uv[1]) + (uz * uv[0] - ux * uv[2]);
        t[2] += (tl[2] + w * uv[2]) + (ux * uv[1] - uy * uv[0]);
        const double ax = q[0], ay = q[1], az = q[2], aw = q[3], bx = ql[0], by = ql[1], bz = ql[2], bw = ql[3];
        q[3] = aw * bw - ax * bx - ay * by - az * bz;
        q[0] = aw * bx + ax * bw + ay * bz - az * by;
        q[1] = aw * by - ax * bz + ay * bw + az * bx;
        q[2] = aw * bz + ax * by - ay * bx + az * bw;
    }
    void matrix(double H[12]) const {                      /* 3x4 row-major [R | t], Eigen toRotationMatrix() */
        const double x = q[0], y = q[1], z = q[2], w = q[3];
        H[0] = 1 - 2 * (y * y + z * z); H[1] = 2 * (x * y - z * w);     H[2] = 2 * (x * z + y * w);     H[3] = t[0];
        H[4] = 2 * (x * y + z * w);     H[5] = 1 - 2 * (x * x + z * z); H[6] = 2 * (y * z - x * w);     H[7] = t[1];
        H[8] = 2 * (x * z - y * w);     H[9] = 2 * (y * z + x * w);     H[10] = 1 - 2 * (x * x + y * y); H[11] = t[2];
    }
};

/* The evaluation artefact of src/laserMapping.cpp:2284-2325: one line per frame, H_init^-1 * H as 12 values in
 * scientific notation with precision 6, appended to RESULT_PATH. */
class TrajectoryWriter {
public:
    explicit TrajectoryWriter(const std::string &result_path) : path_(result_path) {}
    /* a trajectory continued in another process (lane checkpoints): H_init [12] of the file's first pose, as init() gave it */
    TrajectoryWriter(const std::string &result_path, const double *H_init) : path_(result_path), init_flag_(false) { std::copy(H_init, H_init + 12, Hinit_); }
    bool started() const { return !init_flag_; }
    const double *init() const { return Hinit_; }
    void append(const WorldPose &p) {
        double H[12]; p.matrix(H);
        if (init_flag_) { for (int i = 0; i < 12; ++i) Hinit_[i] = H[i]; init_flag_ = false; }
        /* H_init^-1 * H for rigid transforms: R0^T R, R0^T (t - t0) */
        double out[12];
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) out[r * 4 + c] = Hinit_[0 * 4 + r] * H[0 * 4 + c] + Hinit_[1 * 4 + r] * H[1 * 4 + c] + Hinit_[2 * 4 + r] * H[2 * 4 + c];
            out[r * 4 + 3] = Hinit_[0 * 4 + r] * (H[3] - Hinit_[3]) + Hinit_[1 * 4 + r] * (H[7] - Hinit_[7]) + Hinit_[2 * 4 + r] * (H[11] - Hinit_[11]);
        }
        std::FILE *f = std::fopen(path_.c_str(), "a");
        if (!f) throw Error(LL_ERR_ARG, "cannot open " + path_);
        for (int i = 0; i < 12; ++i) std::fprintf(f, i == 11 ? "%.6e\n" : "%.6e ", out[i]);
        std::fclose(f);
    }
private:
    std::string path_;
    bool init_flag_ = true;
    double Hinit_[12];
};

/* laserOdometry over a whole sequence of registered scans in slots [first, first+count): the reference's frame loop
 * (3 outer iterations x ceres::Solve, vote from the 6th frame, warm start) -- ll_odometry_frames. */
inline std::vector<double> odometry_frames(Context &c, int first, int count, const double *pose0 = nullptr, int first_frame_index = 1)
{
    std::vector<double> rel((size_t)count * 7);
    c.check(ll_odometry_frames(c.get(), first, count, pose0, 3, first_frame_index, nullptr, rel.data()));
    return rel;
}

/* laserOdometry for L.n_seq sequences side by side over rows [row0, row0 + n_rows) of a ring (ll_odometry_sequences): returns the
 * [n_rows][S][7] relative poses, NaN for the rows a sequence did not run.  seq_rows / frame_index0 / pose0: NULL or S entries
 * (pose0: S x 7; NULL continues from the poses on the device). */
inline std::vector<double> odometry_sequences(Context &c, const ll_seq_layout &L, int row0, int n_rows, const int *seq_rows = nullptr,
                                              const int *frame_index0 = nullptr, const double *pose0 = nullptr, int n_outer = 3)
{
    std::vector<double> rel((size_t)(n_rows > 0 ? n_rows : 0) * (size_t)(L.n_seq > 0 ? L.n_seq : 0) * 7);
    c.check(ll_odometry_sequences(c.get(), &L, row0, n_rows, seq_rows, frame_index0, pose0, n_outer, nullptr, rel.data()));
    return rel;
}

/* Whole drives side by side (ll_drives): S lanes, each running one drive at a time through registration -> odometry -> mapping,
 * the chain of tools/ll_odometry_kitti with mapping = 1 for every lane in one step.  Upload lane q's raw scan into slots()[q], then
 * step(cmd) with LL_DRIVE_IDLE / LL_DRIVE_RUN / LL_DRIVE_START per lane; odom / mapped ([S][7], NaN for lanes that did not run)
 * and ran ([S]) hold the step's results.  Lane q equals its drive run alone through odometry_frames, WorldPose and a LaserMapping. */
class Drives {
public:
    Drives(Context &c, int n_lanes, int max_scan_corner, int max_scan_surf, int pool_points = 1 << 22, int base = 0, bool keep_registered = false,
           float lineRes = 0.4f, float planeRes = 0.8f, int n_outer = 3)
        : S(n_lanes), odom((size_t)7 * (n_lanes > 0 ? n_lanes : 0)), mapped((size_t)7 * (n_lanes > 0 ? n_lanes : 0)), ran((size_t)(n_lanes > 0 ? n_lanes : 0), 0) {
        ll_drives_params p;
        p.n_lanes = n_lanes; p.base = base; p.line_res = lineRes; p.plane_res = planeRes;
        p.max_scan_corner = max_scan_corner; p.max_scan_surf = max_scan_surf; p.pool_points = pool_points;
        p.n_outer = n_outer; p.keep_registered = keep_registered ? 1 : 0;
        c.check(ll_drives_create(c.get(), &p, &d_));
    }
    ~Drives() { ll_drives_destroy(d_); }
    Drives(const Drives &) = delete;
    Drives &operator=(const Drives &) = delete;

    std::vector<int> slots() {
        std::vector<int> s((size_t)S);
        check(ll_drives_slots(d_, s.data()));
        return s;
    }
    /* cmd: one command per lane; pose0: NULL or [S][7] (the rows of START lanes: the odometry warm start of frame 1) */
    void step(const std::vector<int> &cmd, const double *pose0 = nullptr) {
        if ((int)cmd.size() != S) throw Error(LL_ERR_ARG, "one command per lane");
        check(ll_drives_step(d_, cmd.data(), pose0, odom.data(), mapped.data(), ran.data()));
    }
    /* map_of[q] = -1: lane q maps into its own map (the state after construction); m >= 0: it localises against lane m's map and
     * writes none, from the next step on.  start: NULL or [S][7], the map-to-odom pose LL_DRIVE_START gives a localising lane --
     * where its drive begins in the map.  A step that would map into a map a running lane reads is refused (LL_ERR_ARG) */
    void set_localize(const std::vector<int> &map_of, const double *start = nullptr) {
        if ((int)map_of.size() != S) throw Error(LL_ERR_ARG, "one map per lane");
        check(ll_drives_set_localize(d_, map_of.data(), start));
    }
    /* the mapping lanes vote their plane blocks in frames whose per-lane index is > from_frame (the reference's gate: 20); negative: off.
     * Not part of a checkpoint: set it again after restore */
    void set_map_vote(int from_frame) { check(ll_drives_set_map_vote(d_, from_frame)); }
    /* from the next step on every lane that ran a frame whose per-lane index is a multiple of `every` is captured into kf (its stack
     * clouds and mapped pose, tagged with lane and frame index); nullptr: off.  A step for which the store has no room is refused
     * (LL_ERR_CAPACITY) before it runs.  Not part of a checkpoint */
    void set_keyframes(Keyframes *kf, int every = 1) { check(ll_drives_set_keyframes(d_, kf ? kf->get() : nullptr, every)); }
    /* the map-to-odom pose of every lane with lanes[q] != 0 left-multiplied by C_w7[q] ([S][7]): with C = P'_last o P_last^-1 the lane's
     * drive continues in a map rebuilt under corrected poses.  Between any two steps */
    void correct(const std::vector<int> &lanes, const double *C_w7) {
        if ((int)lanes.size() != S) throw Error(LL_ERR_ARG, "one selection per lane");
        check(ll_drives_correct(d_, lanes.data(), C_w7));
    }
    /* the last step's fit records [S]: zeros for lanes that mapped, sat out or did not optimise */
    std::vector<ll_localize_fit> fit() {
        std::vector<ll_localize_fit> f((size_t)S);
        check(ll_drives_fit(d_, f.data()));
        return f;
    }
    /* the localising lanes' steps also fill information records (off after create; not part of a checkpoint) */
    void set_info(bool on) { check(ll_drives_set_info(d_, on ? 1 : 0)); }
    /* the last step's information records [S]: zeros for lanes that mapped, sat out or did not optimise, and while set_info is off */
    std::vector<PoseInfo> info() {
        std::vector<PoseInfo> f((size_t)S, PoseInfo());
        check(ll_drives_info(d_, f.data()));
        return f;
    }
    /* lane q's mapped pose of the last step, as the trajectory file takes it */
    WorldPose mapped_pose(int q) const {
        WorldPose w;
        for (int i = 0; i < 4; ++i) w.q[i] = mapped[(size_t)7 * q + i];
        for (int i = 0; i < 3; ++i) w.t[i] = mapped[(size_t)7 * q + 4 + i];
        return w;
    }
    /* /velodyne_cloud_registered of lane q from the last step (keep_registered) */
    std::vector<PointXYZI> registered(int q) {
        int n = 0;
        check(ll_drives_registered(d_, q, nullptr, 0, &n));
        std::vector<PointXYZI> out((size_t)n);
        check(ll_drives_registered(d_, q, (ll_point *)out.data(), n, &n));
        return out;
    }
    /* LaserMappingSequences::export_maps of the lanes' maps, between any two steps */
    void export_maps(const std::vector<int> &which, std::vector<PointXYZI> &out, std::vector<long long> &offset) {
        if ((int)which.size() != S) throw Error(LL_ERR_ARG, "one selection per lane");
        const int rc = LaserMappingSequences::export_from(cubemaps(), S, which.data(), out, offset);
        if (rc != LL_OK) throw Error(rc, ll_cubemaps_last_error(cubemaps()));
    }
    /* the checkpoint of the lanes with lanes[q] != 0 (ll_drives_save: one pack launch, one copy, one synchronisation; read-only).
     * A lane can be saved when it ran on the previous step, or was restored and has not stepped since */
    std::vector<unsigned char> save(const std::vector<int> &lanes) {
        if ((int)lanes.size() != S) throw Error(LL_ERR_ARG, "one selection per lane");
        const long long n = ll_drives_save_size(d_, lanes.data());
        if (n < 0) check((int)n);
        std::vector<unsigned char> blob((size_t)n);
        long long got = 0;
        check(ll_drives_save(d_, lanes.data(), blob.data(), n, &got));
        blob.resize((size_t)got);
        return blob;
    }
    /* record r of the checkpoint into lane into[r] (-1: skipped): the lane may then RUN on, bit for bit as if it had never stopped */
    void restore(const std::vector<unsigned char> &blob, const std::vector<int> &into) {
        ll_checkpoint_info info;
        std::memset(&info, 0, sizeof(info));
        if (ll_checkpoint_describe(blob.data(), (long long)blob.size(), &info) == LL_OK && (int)into.size() != info.n_records)
            throw Error(LL_ERR_ARG, "one destination per record");
        check(ll_drives_restore(d_, into.data(), blob.data(), (long long)blob.size()));
    }
    void stats(long long &syncs, long long &frames) const { check(ll_drives_stats(d_, &syncs, &frames)); }
    ll_cubemaps *cubemaps() const { return ll_drives_cubemaps(d_); }
    ll_drives *get() const { return d_; }
    const int S;
    std::vector<double> odom, mapped;   /* [S][7] */
    std::vector<int> ran;               /* [S] */
private:
    void check(int rc) const { if (rc != LL_OK) throw Error(rc, ll_drives_last_error(d_)); }
    ll_drives *d_ = nullptr;
};

/* Place recognition (ll_places): Scan Context descriptors of resident or uploaded scans, 20 rings x 60 sectors = 1200 floats each, and
 * the exact search of every query against every stored place.  Ids are 0 .. size() - 1 in the order of the adds.  With Drives:
 * add_slots takes the values Drives::slots() returned BEFORE the step, after the step.  Destroy it before its Context. */
class Places {
public:
    struct Match { std::vector<int> id; std::vector<float> dist; std::vector<unsigned char> shift; };   /* [nq][K], or [nq][nc] without id */
    Places(Context &c, int capacity, float max_radius = 80.0f, float z_offset = 2.0f) {
        ll_places_params p;
        ll_places_default_params(&p, capacity);
        p.max_radius = max_radius; p.z_offset = z_offset;
        c.check(ll_places_create(c.get(), &p, &db_));
    }
    ~Places() { ll_places_destroy(db_); }
    Places(const Places &) = delete;
    Places &operator=(const Places &) = delete;

    int size() const { return ll_places_size(db_); }
    void reset() { check(ll_places_reset(db_)); }
    /* one place per slot from its laserCloud; the first new id */
    int add_slots(const std::vector<int> &slots) {
        int first = -1;
        check(ll_places_add_slots(db_, slots.data(), (int)slots.size(), &first));
        return first;
    }
    int add_points(const std::vector<PointXYZI> &cloud) {
        int id = -1;
        check(ll_places_add_points(db_, (const ll_point *)cloud.data(), (int)cloud.size(), &id));
        return id;
    }
    /* desc: a multiple of 1200 floats, to ids first .. (first <= size(): overwrites or extends) */
    void upload(int first, const std::vector<float> &desc) {
        if (desc.size() % 1200 != 0) throw Error(LL_ERR_ARG, "descriptors are 1200 floats each");
        check(ll_places_upload(db_, first, (int)(desc.size() / 1200), desc.data()));
    }
    std::vector<float> download(int first, int count) {
        std::vector<float> desc((size_t)1200 * (count > 0 ? count : 0));
        check(ll_places_download(db_, first, count, desc.data()));
        return desc;
    }
    /* every query q0 .. q0 + nq - 1 against every candidate c0 .. c0 + nc - 1: dist and shift [nq][nc] */
    Match distances(int q0, int nq, int c0, int nc) {
        Match m;
        const size_t n = (size_t)(nq > 0 ? nq : 0) * (size_t)(nc > 0 ? nc : 0);
        m.dist.resize(n); m.shift.resize(n);
        check(ll_places_distances(db_, q0, nq, c0, nc, m.dist.data(), m.shift.data()));
        return m;
    }
    /* per query its K best candidates by (distance, id); ranks without one hold (-1, inf, 0).  c_end: empty, or [nq] -- query q only
     * sees candidate ids below c_end[q] */
    Match match(int q0, int nq, int c0, int nc, int K = 1, const std::vector<int> &c_end = std::vector<int>()) {
        if (!c_end.empty() && (int)c_end.size() != nq) throw Error(LL_ERR_ARG, "one c_end per query");
        Match m;
        const size_t n = (size_t)(nq > 0 ? nq : 0) * (size_t)(K > 0 ? K : 0);
        m.id.resize(n); m.dist.resize(n); m.shift.resize(n);
        check(ll_places_match(db_, q0, nq, c0, nc, c_end.empty() ? nullptr : c_end.data(), K, m.id.data(), m.dist.data(), m.shift.data()));
        return m;
    }
    /* ms[3]: the last add / upload, the last search's Gram matrices and diagonals, the last match's selection; counts[2]: places, pairs */
    void timing(double ms[3], long long counts[2]) { check(ll_places_timing(db_, ms, counts)); }
    ll_places *get() const { return db_; }
private:
    void check(int rc) const { if (rc != LL_OK) throw Error(rc, ll_places_last_error(db_)); }
    ll_places *db_ = nullptr;
};

/* Pose graphs (ll_posegraphs): many independent SE(3) graphs optimised side by side, one workgroup per graph.  A Graph holds poses
 * [N][7] (pose_w7, world from body), edges whose i, j index its own poses and whose Z measures P_i^-1 P_j, and an optional fixed flag
 * per node (empty: node 0 is fixed).  An odometry edge's sqrt_info is the caller's choice; the weight of a loop or session edge can be
 * MEASURED: edge_from_info turns the PoseInfo of the localisation or alignment behind it into a full 6 x 6 square-root information
 * (Graph6 / edge6).  Destroy it before its Context. */
class PoseGraphs {
public:
    struct Graph { std::vector<double> poses; std::vector<ll_pg_edge> edges; std::vector<unsigned char> fixed; };
    struct Graph6 { std::vector<double> poses; std::vector<ll_pg_edge6> edges; std::vector<unsigned char> fixed; };   /* full-information edges */
    struct Evaluation { std::vector<double> cost; std::vector<std::vector<double>> grad; };   /* [graphs], [graphs][N * 6] */
    PoseGraphs(Context &c, int max_graphs, int max_nodes_total, int max_edges_total) {
        c.check(ll_posegraphs_create(c.get(), max_graphs, max_nodes_total, max_edges_total, &pg_));
    }
    ~PoseGraphs() { ll_posegraphs_destroy(pg_); }
    PoseGraphs(const PoseGraphs &) = delete;
    PoseGraphs &operator=(const PoseGraphs &) = delete;

    static ll_pg_options default_options() { ll_pg_options o; ll_pg_default_options(&o); return o; }
    /* P_i^-1 P_j in the pose_w7 layout: the measurement of an odometry edge between two poses of a chain */
    static void relative_pose(const double Pi[7], const double Pj[7], double Z[7]) {
        const double ci[4] = {-Pi[0], -Pi[1], -Pi[2], Pi[3]}, v[3] = {Pj[4] - Pi[4], Pj[5] - Pi[5], Pj[6] - Pi[6]};
        qmul(ci, Pj, Z);
        const double tq[4] = {v[0], v[1], v[2], 0.0};
        double a[4], b[4];
        const double n2 = Pi[0] * Pi[0] + Pi[1] * Pi[1] + Pi[2] * Pi[2] + Pi[3] * Pi[3];
        qmul(ci, tq, a); qmul(a, Pi, b);                                    /* q* v q = R(q)^T v |q|^2 */
        for (int k = 0; k < 3; ++k) Z[4 + k] = b[k] / n2;
    }
    static ll_pg_edge edge(int i, int j, const double Z[7], double sqrt_info_rot, double sqrt_info_trans, double huber = 0.0) {
        ll_pg_edge e;
        e.i = i; e.j = j; e.huber = huber;
        for (int k = 0; k < 7; ++k) e.Z_w7[k] = Z[k];
        for (int k = 0; k < 3; ++k) { e.sqrt_info[k] = sqrt_info_rot; e.sqrt_info[3 + k] = sqrt_info_trans; }
        return e;
    }
    /* an edge with the full square-root information S [36] (row-major, r = S e) */
    static ll_pg_edge6 edge6(int i, int j, const double Z[7], const double S[36], double huber = 0.0) {
        ll_pg_edge6 e;
        e.i = i; e.j = j; e.huber = huber;
        for (int k = 0; k < 7; ++k) e.Z_w7[k] = Z[k];
        for (int k = 0; k < 36; ++k) e.S[k] = S[k];
        return e;
    }
    /* a diagonal edge as a full one: S = diag(sqrt_info) */
    static ll_pg_edge6 edge6(const ll_pg_edge &d) {
        ll_pg_edge6 e;
        e.i = d.i; e.j = d.j; e.huber = d.huber;
        for (int k = 0; k < 7; ++k) e.Z_w7[k] = d.Z_w7[k];
        for (int k = 0; k < 36; ++k) e.S[k] = (k % 7 == 0) ? d.sqrt_info[k / 7] : 0.0;
        return e;
    }
    /* ll_pg_edge_from_info: S [36] of the edge (i, j, Z = P_i^-1 X) whose measurement the record describes; X: the localised pose or the
     * aligned T; sigma: the residual standard deviation in metres (<= 0: sqrt(info.sigma2)); floor: added to the information's diagonal */
    static void edge_from_info(const PoseInfo &info, const double X_w7[7], double sigma, double floor, double S[36]) {
        const int rc = ll_pg_edge_from_info(&info, X_w7, sigma, floor, S);
        if (rc != LL_OK) throw Error(rc, rc == LL_ERR_STATE ? "edge_from_info: the record is not finite, sigma2 is 0 with sigma <= 0, or the information is not positive definite"
                                                            : "edge_from_info: a non-finite argument, a negative floor or a zero quaternion");
    }
    /* the robustified cost of every graph and its gradient per node (6 each, zeros at fixed nodes); solves nothing */
    Evaluation evaluate(const std::vector<Graph6> &graphs) {
        pack(graphs, edges6_);
        Evaluation ev;
        ev.cost.resize(graphs.size());
        std::vector<double> grad(poses_.size() / 7 * 6);
        check(ll_posegraphs_evaluate6(pg_, (int)graphs.size(), node_off_.data(), edge_off_.data(), poses_.data(), fixed_ptr(), edges6_.data(),
                                      ev.cost.data(), grad.data()));
        for (size_t g = 0; g < graphs.size(); ++g)
            ev.grad.emplace_back(grad.begin() + (size_t)node_off_[g] * 6, grad.begin() + (size_t)node_off_[g + 1] * 6);
        return ev;
    }
    std::vector<ll_pg_record> solve(std::vector<Graph6> &graphs, const ll_pg_options *opt = nullptr) {
        pack(graphs, edges6_);
        std::vector<ll_pg_record> rec(graphs.size());
        check(ll_posegraphs_solve6(pg_, (int)graphs.size(), node_off_.data(), edge_off_.data(), poses_.data(), fixed_ptr(), edges6_.data(), opt, rec.data()));
        for (size_t g = 0; g < graphs.size(); ++g)
            std::copy(poses_.begin() + (size_t)node_off_[g] * 7, poses_.begin() + (size_t)node_off_[g + 1] * 7, graphs[g].poses.begin());
        return rec;
    }
    Evaluation evaluate(const std::vector<Graph> &graphs) {
        pack(graphs, edges_);
        Evaluation ev;
        ev.cost.resize(graphs.size());
        std::vector<double> grad(poses_.size() / 7 * 6);
        check(ll_posegraphs_evaluate(pg_, (int)graphs.size(), node_off_.data(), edge_off_.data(), poses_.data(), fixed_ptr(), edges_.data(),
                                     ev.cost.data(), grad.data()));
        for (size_t g = 0; g < graphs.size(); ++g)
            ev.grad.emplace_back(grad.begin() + (size_t)node_off_[g] * 6, grad.begin() + (size_t)node_off_[g + 1] * 6);
        return ev;
    }
    /* optimises every graph's poses in place; one record per graph */
    std::vector<ll_pg_record> solve(std::vector<Graph> &graphs, const ll_pg_options *opt = nullptr) {
        pack(graphs, edges_);
        std::vector<ll_pg_record> rec(graphs.size());
        check(ll_posegraphs_solve(pg_, (int)graphs.size(), node_off_.data(), edge_off_.data(), poses_.data(), fixed_ptr(), edges_.data(), opt, rec.data()));
        for (size_t g = 0; g < graphs.size(); ++g)
            std::copy(poses_.begin() + (size_t)node_off_[g] * 7, poses_.begin() + (size_t)node_off_[g + 1] * 7, graphs[g].poses.begin());
        return rec;
    }
    /* ms[2]: the last evaluate, the last solve (device time); counts[3]: graphs, LM iterations, PCG iterations of the last call */
    void timing(double ms[2], long long counts[3]) { check(ll_posegraphs_timing(pg_, ms, counts)); }
    /* LL_PG_PRECOND_BLOCK_JACOBI (the default) or LL_PG_PRECOND_CHAIN: the preconditioner of the solves from the next call on */
    void set_preconditioner(int kind) { check(ll_posegraphs_set_preconditioner(pg_, kind)); }
    int preconditioner() const { return ll_posegraphs_preconditioner(pg_); }
    /* counts[2]: factorisations of the chain matrix, LM iterations that fell back to block-Jacobi, over the graphs of the last solve */
    void precond_stats(long long counts[2]) { check(ll_posegraphs_precond_stats(pg_, counts)); }
    /* ll_posegraphs_chain_solve: block-tridiagonal SPD systems back to back; diag36, upper36 [nodes][36], rhs6 [nodes][6] -> x [nodes][6];
     * status[s] is 1 where a pivot of system s failed (its x is zeros) */
    struct ChainSolution { std::vector<double> x; std::vector<int> status; };
    ChainSolution chain_solve(const std::vector<int> &node_off, const std::vector<double> &diag36, const std::vector<double> &upper36,
                              const std::vector<double> &rhs6) {
        if (node_off.empty()) throw Error(LL_ERR_ARG, "node_off has one entry per system and one more");
        const size_t n = (size_t)node_off.back();
        if (diag36.size() != n * 36 || upper36.size() != n * 36 || rhs6.size() != n * 6) throw Error(LL_ERR_ARG, "36, 36 and 6 doubles per node");
        ChainSolution s;
        s.x.assign(n * 6, 0.0); s.status.assign(node_off.size() - 1, 0);
        check(ll_posegraphs_chain_solve(pg_, (int)node_off.size() - 1, node_off.data(), diag36.data(), upper36.data(), rhs6.data(), s.x.data(), s.status.data()));
        return s;
    }
    /* ll_posegraphs_covariances: joint[q * 144 ..] is the row-major 12 x 12 [[S_aa, S_ab], [S_ba, S_bb]] of query q = (graph, a, b) in the
     * increments' tangent (half-angle vector, translation; a rotation-vector covariance is 4 x the rotation block), b < 0: node a alone.
     * records[q].status: 0 converged, 1 a column hit max_pcg_iterations, 2 breakdown (zeros).  The object's preconditioner applies */
    struct Covariances { std::vector<double> joint; std::vector<ll_pg_cov_record> records; };
    static ll_pg_cov_options default_cov_options() { ll_pg_cov_options o; ll_pg_cov_default_options(&o); return o; }
    Covariances covariances(const std::vector<Graph> &graphs, const std::vector<ll_pg_cov_query> &queries, const ll_pg_cov_options *opt = nullptr) {
        pack(graphs, edges_);
        Covariances c;
        c.joint.assign(queries.size() * 144, 0.0); c.records.resize(queries.size());
        check(ll_posegraphs_covariances(pg_, (int)graphs.size(), node_off_.data(), edge_off_.data(), poses_.data(), fixed_ptr(), edges_.data(),
                                        (int)queries.size(), queries.data(), opt, c.joint.data(), c.records.data()));
        return c;
    }
    Covariances covariances(const std::vector<Graph6> &graphs, const std::vector<ll_pg_cov_query> &queries, const ll_pg_cov_options *opt = nullptr) {
        pack(graphs, edges6_);
        Covariances c;
        c.joint.assign(queries.size() * 144, 0.0); c.records.resize(queries.size());
        check(ll_posegraphs_covariances6(pg_, (int)graphs.size(), node_off_.data(), edge_off_.data(), poses_.data(), fixed_ptr(), edges6_.data(),
                                         (int)queries.size(), queries.data(), opt, c.joint.data(), c.records.data()));
        return c;
    }
    /* ms[2]: the last covariances call's prepare and columns (device time); counts[3]: its queries, sources, PCG iterations */
    void cov_timing(double ms[2], long long counts[3]) { check(ll_posegraphs_cov_timing(pg_, ms, counts)); }
    /* ll_pg_edge_gate: chi2 (6 degrees of freedom) of the candidate edge a -> b (Z, S36 or NULL) against the joint covariance of the two
     * poses; C36 (may be NULL) gets J Sigma J^T + (S^T S)^-1.  A chi-square only for an edge that is NOT in the graph.  Needs no device */
    static double edge_gate(const double Pa[7], const double Pb[7], const double Z[7], const double *S36, const double *joint144, double *C36 = nullptr) {
        double chi2 = 0.0;
        const int rc = ll_pg_edge_gate(Pa, Pb, Z, S36, joint144, &chi2, C36);
        if (rc != LL_OK) throw Error(rc, "edge_gate: a non-finite input, a zero quaternion, or a covariance or information that is not positive definite");
        return chi2;
    }
    ll_posegraphs *get() const { return pg_; }
private:
    static void qmul(const double a[4], const double b[4], double o[4]) {
        o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
        o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
        o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
        o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    }
    /* the ragged packing: graphs back to back; a graph without flags gets node 0 fixed */
    template <class G, class E>
    void pack(const std::vector<G> &graphs, std::vector<E> &edges_) {
        node_off_.assign(1, 0); edge_off_.assign(1, 0); poses_.clear(); edges_.clear(); fixed_.clear();
        for (const G &g : graphs) {
            if (g.poses.size() % 7 != 0) throw Error(LL_ERR_ARG, "poses are 7 doubles each");
            const size_t n = g.poses.size() / 7;
            if (!g.fixed.empty() && g.fixed.size() != n) throw Error(LL_ERR_ARG, "one fixed flag per node");
            poses_.insert(poses_.end(), g.poses.begin(), g.poses.end());
            edges_.insert(edges_.end(), g.edges.begin(), g.edges.end());
            for (size_t k = 0; k < n; ++k) fixed_.push_back(g.fixed.empty() ? (unsigned char)(k == 0) : g.fixed[k]);
            node_off_.push_back((int)(poses_.size() / 7)); edge_off_.push_back((int)edges_.size());
        }
    }
    const unsigned char *fixed_ptr() const { return fixed_.data(); }
    void check(int rc) const { if (rc != LL_OK) throw Error(rc, ll_posegraphs_last_error(pg_)); }
    ll_posegraphs *pg_ = nullptr;
    std::vector<int> node_off_, edge_off_;
    std::vector<double> poses_;
    std::vector<ll_pg_edge> edges_;
    std::vector<ll_pg_edge6> edges6_;
    std::vector<unsigned char> fixed_;
};

/* Pcm (ll_pcm): the pairwise-consistent set of loop-closure candidates of many graphs side by side -- over ALL candidates of a revisit,
 * before the gate or a Huber width see the survivors.  A Graph holds poses [N][7] in trajectory order and candidates whose i, j index
 * its own poses and whose Z measures P_i^-1 P_j.  Thresholds, not a Mahalanobis test; a greedy clique, not the maximum one.  Destroy it
 * before its Context. */
class Pcm {
public:
    struct Graph { std::vector<double> poses; std::vector<ll_pcm_candidate> candidates; };
    struct Result { std::vector<std::vector<unsigned char>> selected; std::vector<std::vector<int>> degree; std::vector<ll_pcm_record> rec; };
    Pcm(Context &c, int max_graphs, int max_nodes_total, int max_candidates_total) {
        c.check(ll_pcm_create(c.get(), max_graphs, max_nodes_total, max_candidates_total, &p_));
    }
    ~Pcm() { ll_pcm_destroy(p_); }
    Pcm(const Pcm &) = delete;
    Pcm &operator=(const Pcm &) = delete;

    static ll_pcm_params default_params() { ll_pcm_params p; ll_pcm_default_params(&p); return p; }
    static size_t words(size_t n_candidates) { return (n_candidates + 63) / 64; }
    static ll_pcm_candidate candidate(int i, int j, const double Z[7]) {
        ll_pcm_candidate c;
        c.i = i; c.j = j;
        for (int k = 0; k < 7; ++k) c.Z_w7[k] = Z[k];
        return c;
    }
    /* a pose-graph edge is a candidate as it is */
    static ll_pcm_candidate candidate(const ll_pg_edge &e) { return candidate(e.i, e.j, e.Z_w7); }
    static ll_pcm_candidate candidate(const ll_pg_edge6 &e) { return candidate(e.i, e.j, e.Z_w7); }

    /* ONE synchronisation whatever graphs.size() is */
    Result run(const std::vector<Graph> &graphs, const ll_pcm_params *params = nullptr) {
        std::vector<int> node_off(1, 0), cand_off(1, 0);
        std::vector<double> poses; std::vector<ll_pcm_candidate> cands;
        for (const Graph &g : graphs) {
            poses.insert(poses.end(), g.poses.begin(), g.poses.end());
            cands.insert(cands.end(), g.candidates.begin(), g.candidates.end());
            node_off.push_back((int)(poses.size() / 7)); cand_off.push_back((int)cands.size());
        }
        std::vector<unsigned char> sel(cands.size() + 1); std::vector<int> deg(cands.size() + 1);
        Result r; r.rec.resize(graphs.size());
        check(ll_pcm_run(p_, (int)graphs.size(), node_off.data(), cand_off.data(), poses.data(), cands.data(), params, sel.data(), deg.data(), r.rec.data()));
        split(cand_off, sel, deg, r);
        return r;
    }
    /* the selection alone; matrices[g]: C rows of words(C) 64-bit words, bit d % 64 of word d / 64 of row c standing for (c, d) */
    Result select(const std::vector<std::vector<unsigned long long>> &matrices, const std::vector<int> &n_candidates) {
        std::vector<int> cand_off(1, 0);
        std::vector<unsigned long long> all;
        for (size_t g = 0; g < matrices.size(); ++g) {
            if (matrices[g].size() != (size_t)n_candidates[g] * words((size_t)n_candidates[g])) throw Error(LL_ERR_ARG, "Pcm::select: a matrix of C rows has C * words(C) words");
            all.insert(all.end(), matrices[g].begin(), matrices[g].end());
            cand_off.push_back(cand_off.back() + n_candidates[g]);
        }
        std::vector<unsigned char> sel((size_t)cand_off.back() + 1); std::vector<int> deg((size_t)cand_off.back() + 1);
        Result r; r.rec.resize(matrices.size());
        check(ll_pcm_select(p_, (int)matrices.size(), cand_off.data(), all.data(), sel.data(), deg.data(), r.rec.data()));
        split(cand_off, sel, deg, r);
        return r;
    }
    /* the bit matrix of graph g of the last run or select, n_candidates rows in original order */
    std::vector<unsigned long long> adjacency(int g, int n_candidates) {
        std::vector<unsigned long long> w((size_t)n_candidates * words((size_t)n_candidates) + 1);
        check(ll_pcm_adjacency(p_, g, w.data()));
        w.pop_back();
        return w;
    }
    void timing(double ms[5], long long counts[4]) const { check(ll_pcm_timing(p_, ms, counts)); }
    /* one graph on the host, no device */
    static int host(const Graph &g, const ll_pcm_params *params, std::vector<unsigned long long> *words_out, std::vector<unsigned char> &selected,
                    std::vector<int> *degree, ll_pcm_record *rec) {
        const size_t C = g.candidates.size();
        selected.assign(C + 1, 0);
        if (words_out) words_out->assign(C * words(C) + 1, 0ull);
        if (degree) degree->assign(C + 1, 0);
        const int rc = ll_pcm_host((int)(g.poses.size() / 7), g.poses.data(), (int)C, g.candidates.data(), params, words_out ? words_out->data() : nullptr,
                                   selected.data(), degree ? degree->data() : nullptr, rec);
        selected.resize(C);
        if (words_out) words_out->pop_back();
        if (degree) degree->resize(C);
        return rc;
    }
    ll_pcm *get() const { return p_; }
private:
    void check(int rc) const { if (rc != LL_OK) throw Error(rc, ll_pcm_last_error(p_)); }
    static void split(const std::vector<int> &off, const std::vector<unsigned char> &sel, const std::vector<int> &deg, Result &r) {
        for (size_t g = 0; g + 1 < off.size(); ++g) {
            r.selected.emplace_back(sel.begin() + off[g], sel.begin() + off[g + 1]);
            r.degree.emplace_back(deg.begin() + off[g], deg.begin() + off[g + 1]);
        }
    }
    ll_pcm *p_ = nullptr;
};

}  // namespace lightloam

/* ------------------------------------------------------------------------------------------------------------------
 * Optional Ceres adapter (NOT compiled in this image: Ceres is absent).  Keeps the parameter-block layout (4, 3) of
 * lidarFactor.hpp and lets ceres::Solve drive the device evaluation: ONE cost function for all residual blocks of the
 * frame, whose Evaluate() is ll_residual_jacobian (rows = 3 * edges + selected planes, jacobians[0] rows x 4 over
 * (x,y,z,w), jacobians[1] rows x 3, row-major).  HuberLoss(0.1) is applied per reference residual block, so the batched
 * function must be wrapped with LL huber off and a ceres::LossFunction cannot be used as is -- see INTEGRATION.md.   */
#if defined(LIGHTLOAM_WITH_CERES) && __has_include(<ceres/ceres.h>)
#include <ceres/ceres.h>
namespace lightloam {
class BatchedLidarCost : public ceres::CostFunction {
public:
    BatchedLidarCost(Context &c, int slot, int rows) : c_(c), slot_(slot) {
        set_num_residuals(rows);
        mutable_parameter_block_sizes()->push_back(4);
        mutable_parameter_block_sizes()->push_back(3);
        jq_.resize((size_t)rows * 4); jt_.resize((size_t)rows * 3);
    }
    bool Evaluate(double const *const *parameters, double *residuals, double **jacobians) const override {
        const double pose[7] = {parameters[0][0], parameters[0][1], parameters[0][2], parameters[0][3],
                                parameters[1][0], parameters[1][1], parameters[1][2]};
        if (ll_residual_jacobian(c_.get(), slot_, pose, residuals, jq_.data(), jt_.data(), num_residuals()) != LL_OK) return false;
        if (jacobians && jacobians[0]) std::copy(jq_.begin(), jq_.end(), jacobians[0]);
        if (jacobians && jacobians[1]) std::copy(jt_.begin(), jt_.end(), jacobians[1]);
        return true;
    }
private:
    Context &c_; int slot_;
    mutable std::vector<double> jq_, jt_;
};

/* the same for the mapping blocks of a MapOptimizer after ll_map_associate (LidarEdgeFactor + LidarPlaneNormFactor rows,
 * laserMapping.cpp:1918-1919, :2033-2034); parameter blocks (4, 3) = parameters, parameters + 4 (:1871-1872) */
class BatchedMapCost : public ceres::CostFunction {
public:
    BatchedMapCost(MapOptimizer &m, int rows) : m_(m) {
        set_num_residuals(rows);
        mutable_parameter_block_sizes()->push_back(4);
        mutable_parameter_block_sizes()->push_back(3);
        jq_.resize((size_t)rows * 4); jt_.resize((size_t)rows * 3);
    }
    bool Evaluate(double const *const *parameters, double *residuals, double **jacobians) const override {
        const double pose[7] = {parameters[0][0], parameters[0][1], parameters[0][2], parameters[0][3],
                                parameters[1][0], parameters[1][1], parameters[1][2]};
        if (ll_map_residual_jacobian(m_.get(), pose, residuals, jq_.data(), jt_.data(), num_residuals()) != LL_OK) return false;
        if (jacobians && jacobians[0]) std::copy(jq_.begin(), jq_.end(), jacobians[0]);
        if (jacobians && jacobians[1]) std::copy(jt_.begin(), jt_.end(), jacobians[1]);
        return true;
    }
private:
    MapOptimizer &m_;
    mutable std::vector<double> jq_, jt_;
};
}  // namespace lightloam
#endif

#endif /* LIGHTLOAM_HOST_HPP */
