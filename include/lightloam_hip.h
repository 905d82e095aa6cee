/*
 * lightloam_hip.h -- C ABI of the MI355X-native (gfx950) Light-LOAM per-scan hot path.
 *
 * The reference (BrenYi/Light-LOAM, paths relative to /root/reference/) has no FFI/plugin interface; the
 * seams a replacement sits behind are its node callback, one free function and the Ceres cost-functor
 * factories.  Each entry point below names the reference code it replaces.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no C++/torch types.  Every function returns LL_OK (0) or a
 *    negative ll_status; nothing throws across the boundary.
 *  - ll_ctx owns all device memory and one HIP stream.  One ctx per host thread; not re-entrant
 *    (neither is the reference: file-scope arrays, scanRegistration.cpp:34-40; single-threaded spinner :475).
 *  - A ctx holds `batch` scan SLOTS resident in HBM.  The *_batch entry points run a stage for a
 *    contiguous range of slots in one set of kernel launches (this is how 256 CUs are filled: one scan
 *    is only 64 ring-sized work items).  The single-scan convenience calls at the end operate on slot 0.
 *  - Points are pcl::PointXYZI packed to 16 B: x, y, z, intensity (= scanID + 0.1*relTime,
 *    scanRegistration.cpp:208).  Quaternions are (x, y, z, w) like para_q (laserOdometry.cpp:61).
 *  - "host" pointers are ordinary host memory; they are copied on the ctx stream and the call returns
 *    after the copy completed.  Device-resident use: upload once, run stages, download what is needed.
 *  - There is no CPU fallback: if no gfx950 device/HIP runtime is usable, ll_create fails with LL_ERR_DEVICE.
 */
#ifndef LIGHTLOAM_HIP_H
#define LIGHTLOAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LL_ABI_VERSION 3          /* 2: ll_params.distortion; 3: ll_params.voxel_sort_ranks, .input_stride_floats */

typedef struct ll_ctx ll_ctx;

typedef struct { float x, y, z, intensity; } ll_point;     /* pcl::PointXYZI, common.h:7 */

typedef enum {
    LL_OK = 0,
    LL_ERR_DEVICE = -1,       /* no usable HIP device / kernel image (product path never falls back to CPU) */
    LL_ERR_ARG = -2,
    LL_ERR_BAD_RINGS = -3,    /* scan_line not in {16,32,64} with ring_model 0: ROS_BREAK / return 0 in the reference
                                 (scanRegistration.cpp:170-174, :447-451) */
    LL_ERR_CAPACITY = -4,     /* more points than max_points (reference: fixed 400000 arrays, :34-40) or a ring
                                 longer than max_ring_points */
    LL_ERR_EMPTY = -5,        /* no point survives the NaN / minimum-range filters (reference dereferences points[0]) */
    LL_ERR_HIP = -6,          /* a HIP runtime call failed; ll_last_error() has the text */
    LL_ERR_STATE = -7         /* stage called before its inputs exist (e.g. associate before set_target) */
} ll_status;

/* Node parameters (scanRegistration.cpp:435-443, laserOdometry.cpp:23-30) + capacities. */
typedef struct {
    int   n_scans;            /* "scan_line": 16 / 32 / 64 */
    int   ring_model;         /* 0: reference switch on n_scans; 1: the linear 64-ring formula (:162) for any n_scans */
    float minimum_range;      /* "minimum_range" (launch: 5 for HDL-64, 0.3 for VLP-16/HDL-32) */
    float lower_bound;        /* "lowerBound" default -24.9 */
    float up_bound;           /* "upBound" default 2 */
    int   max_points;         /* per-scan point capacity (<= 400000 like the reference arrays) */
    int   max_ring_points;    /* per-ring capacity, 32 .. 8192 (default 2304): the feature kernel's LDS staging, and the stride at which
                                 the rings of laserCloud sit in HBM (n_scans x max_ring_points points per slot) */
    int   batch;              /* scan slots resident in HBM */
    /* thresholds; ll_default_params() fills the reference constants */
    float curv_threshold;     /* 0.1  (:266, :321) compared as double like the reference */
    float gap_sq_threshold;   /* 0.05 (:293 ...) */
    float leaf_size;          /* 0.2  (:373) */
    float nn_dist_sq_max;     /* DISTANCE_SQ_THRESHOLD 25 (laserOdometry.cpp:29) */
    float nearby_scan;        /* NEARBY_SCAN 2.5 (laserOdometry.cpp:30) */
    float huber_delta;        /* HuberLoss(0.1) (laserOdometry.cpp:475); <= 0 disables the loss */
    int   write_curvature;    /* also store cloudCurvature[] to HBM (debug / parity output; off on the hot path) */
    int   chunk;              /* ll_hot_path_batch processes the slot range in chunks of this many scans so that a chunk's
                                 intermediates stay in the 256 MiB Infinity Cache between kernels; 0 = whole range */
    int   distortion;         /* DISTORTION of laserOdometry.cpp:23.  0 (default) = the reference's build: s = 1.  1 = its other compile-time
                                 path: every point's interpolation ratio s = (intensity - int(intensity)) / SCAN_PERIOD in TransformToStart
                                 (:81-88) and in LidarEdgeFactor / LidarPlaneFactor_modify (:570-571, :740-741, lidarFactor.hpp:25-27) */
    int   voxel_sort_ranks;   /* the VoxelGrid sort's ranking (ll_features.hip).  0 (default) = auto: ranks from one returning LDS add per row when
                                 the device passes ll_create's lane-order check, else from a match-any; 1 = always the match-any (tests; same clouds
                                 bit for bit, ~0.7 % of that kernel slower) */
    int   input_stride_floats;/* floats per point of the RESIDENT raw scan: 4 (default; KITTI .bin, PointXYZ: x, y, z, one unused float) or 3
                                 (x, y, z packed: scanRegistration.cpp:105-106 keeps nothing else, so a streamed scan crosses PCIe and is read by
                                 the organise stage at 12 instead of 16 bytes per point).  ll_upload_scan repacks any caller stride into it; the
                                 asynchronous uploads take their buffers in exactly this layout */
} ll_params;

/* Per-scan sizes produced by the extract stage. */
typedef struct {
    int status;               /* ll_status of this slot's last extract */
    int n_in;                 /* points uploaded */
    int n;                    /* laserCloud size after filtering + ring rejection (cloudSize, :212) */
    int n_sharp, n_less_sharp, n_flat, n_less_flat;
    int max_ring;             /* longest ring */
} ll_scan_info;

/* Per-pair sizes produced by associate / vote. */
typedef struct {
    int n_edge;               /* corner_correspondence (laserOdometry.cpp:617) */
    int n_plane;              /* plane_correspondence (:790) */
    int n_plane_selected;     /* selected_idx.size() after the vote (:796); == n_plane when vote disabled */
} ll_pair_info;

/* ---------------------------------------------------------------- lifecycle */
void        ll_default_params(ll_params *p, int n_scans);
/* ll_create: LL_ERR_ARG for parameters outside their ranges, LL_ERR_DEVICE when `device` is no usable gfx950 device -- the library has no CPU path
 * --, LL_ERR_HIP when an allocation fails or the one-off lane-order check of the voxel filter's sort could not run (a device that fails the check
 * itself is served by the sort's other ranking, ll_params.voxel_sort_ranks); ll_last_error(NULL) says which. */
int         ll_create(int device, const ll_params *p, ll_ctx **out);
void        ll_destroy(ll_ctx *ctx);
const char *ll_last_error(const ll_ctx *ctx);      /* ctx may be NULL: last create error */
int         ll_abi_version(void);
void       *ll_stream(ll_ctx *ctx);                 /* hipStream_t the ctx launches on (for HIP-event timing) */
int         ll_synchronize(ll_ctx *ctx);

/* ---------------------------------------------------------------- input
 * Replaces pcl::fromROSMsg of the /rslidar_points message (scanRegistration.cpp:105-106, :453).
 * xyz: n points of `stride_floats` floats each (>= 3; 4 = KITTI .bin / PointXYZ padding).              */
int ll_upload_scan(ll_ctx *ctx, int slot, const float *host_xyz, int stride_floats, int n);
/* Streaming input (BASELINE config 5): the same upload, asynchronous on the context's COPY stream.  xyz4: n points in the context's RESIDENT
 * layout -- (x, y, z, .) at a 16-byte stride by default, (x, y, z) packed at 12 bytes with ll_params.input_stride_floats = 3 (nothing is
 * repacked on the way: a quarter fewer bytes cross PCIe) --, ideally page-locked (ll_host_alloc); it must not be modified until the copy has run.  The copy
 * stream (1) and the compute stream (0: every stage call) are ordered by caller-named events 0 .. 7, never by blocking the
 * host: ll_stream_record marks "everything enqueued on that stream so far", ll_stream_wait makes what is enqueued on a stream
 * from now on wait for a mark (a never-recorded event: no wait).  Slots in two halves + two events per half = a double
 * buffer: the upload of one half overlaps the processing of the other (bench.py --stream-input).                         */
#define LL_STREAM_COMPUTE 0
#define LL_STREAM_COPY 1
int   ll_upload_scan_async(ll_ctx *ctx, int slot, const float *xyz4, int n);
int   ll_upload_scans_async(ll_ctx *ctx, int first, int count, const float *const *xyz4, const int *n);   /* slots first .. first+count-1 */
/* the same for a run of slots out of ONE page-locked staging area, scan i at base + i * stride_bytes (stride a multiple of 16; of 4 in the
 * 12-byte layout):
 * two enqueues for the whole run (a per-scan feed is bounded by the host cost of the copy calls, not by PCIe) */
int   ll_upload_scans_async_strided(ll_ctx *ctx, int first, int count, const float *base, size_t stride_bytes, const int *n);
int   ll_stream_record(ll_ctx *ctx, int stream, int event_id);
int   ll_stream_wait(ll_ctx *ctx, int stream, int event_id);
int   ll_synchronize_copy(ll_ctx *ctx);
void *ll_host_alloc(size_t bytes);            /* page-locked host memory (NULL on failure) */
void  ll_host_free(void *p);


/* ---------------------------------------------------------------- a1-a4: laserCloudHandler
 * scanRegistration.cpp:87-428 for slots [first, first+count): removeNaN + removeClosedPointCloud (:58-85,
 * :109-110), ring / relTime assignment and stable ring bucketing (:113-221), curvature (:225-235),
 * per-segment sort + greedy pick (:246-368), per-ring VoxelGrid of the less-flat points (:370-376).
 * Per-slot failures (empty scan, capacity) are reported in ll_scan_info.status; the call itself
 * fails only on argument / runtime errors.                                                            */
int ll_extract_batch(ll_ctx *ctx, int first, int count);
int ll_get_scan_info(ll_ctx *ctx, int slot, ll_scan_info *info);

/* Downloads (what the node publishes, :382-410, plus the file-scope arrays for parity checks).
 * Any pointer may be NULL.  Capacities are in elements; LL_ERR_CAPACITY if too small.                  */
int ll_download_cloud(ll_ctx *ctx, int slot, ll_point *cloud, int cap, int *scan_start, int *scan_end /* n_scans each */);
int ll_download_labels(ll_ctx *ctx, int slot, int8_t *label, float *curvature /* needs write_curvature */, int cap);
int ll_download_features(ll_ctx *ctx, int slot,
                         ll_point *sharp, int cap_sharp, ll_point *less_sharp, int cap_less_sharp,
                         ll_point *flat, int cap_flat, ll_point *less_flat, int cap_less_flat);

/* ---------------------------------------------------------------- a5-a7: data association
 * Replaces the kd-tree rebuild (laserOdometry.cpp:882-896) + the two correspondence loops (:491-620, :653-793)
 * for pairs (slot k, its target).  Targets of slot k are the less-sharp / less-flat clouds of slot k-1;
 * slot `first`'s target is the ctx "carry" target (the previous batch's last scan, or whatever
 * ll_set_target uploaded).  pose_guess: count x 7 doubles (qx,qy,qz,qw,tx,ty,tz) = para_q/para_t at entry
 * (:61-62); NULL = identity.
 * The association FIXES a slot's target: ll_vote_batch, ll_normal_equations_batch, ll_residual_jacobian and the solves read
 * whose points the slot's correspondences name from what ll_associate_batch recorded, so a later call over any sub-range
 * (e.g. ll_vote_batch(k, 1)) refers to the same clouds.                                                                */
int ll_set_target(ll_ctx *ctx, const ll_point *host_corner_last, int m_c, const ll_point *host_surf_last, int m_s);
/* The four feature clouds of a scan from host memory into a slot, in place of ll_extract_batch: what a separate
 * laserOdometry process receives on /laser_cloud_sharp, _less_sharp, _flat, _less_flat (laserOdometry.cpp:116-150,
 * :404-423) when the registration node runs elsewhere.  The slot then serves ll_associate_batch .. ll_odometry_frames and
 * ll_set_target_from_slot like an extracted one (its laserCloud / labels are empty).  intensity must carry the ring id
 * as the registration node stores it (int part = scanID).  LL_ERR_CAPACITY beyond the per-scan feature capacities.     */
int ll_upload_features(ll_ctx *ctx, int slot, const ll_point *host_sharp, int n_sharp, const ll_point *host_less_sharp, int n_less_sharp,
                       const ll_point *host_flat, int n_flat, const ll_point *host_less_flat, int n_less_flat);
int ll_set_target_from_slot(ll_ctx *ctx, int slot);   /* device-to-device: slot's less-sharp/less-flat become the carry */
int ll_associate_batch(ll_ctx *ctx, int first, int count, const double *host_pose_guess);
/* Store the guess in HBM; ll_hot_path_batch(..., NULL, ...) then restarts every slot from it without touching the host. */
int ll_set_pose_guess(ll_ctx *ctx, int first, int count, const double *host_pose_guess);
int ll_get_pair_info(ll_ctx *ctx, int slot, ll_pair_info *info);
/* edge: (src index into sharp, a, b into corner_last); plane: (src into flat, a, b, c into surf_last).  */
int ll_download_edge_corr(ll_ctx *ctx, int slot, int *src, int *a, int *b, int cap);
int ll_download_plane_corr(ll_ctx *ctx, int slot, int *src, int *a, int *b, int *c, int cap);

/* ---------------------------------------------------------------- a8: graph vote
 * graph_based_correspondence_vote_simple (laserOdometry.cpp:165-342, call :796) on the plane
 * correspondences of each pair.  enable = 0 reproduces the now_frame <= 5 branch (:781-787): all kept, weight 1. */
int ll_vote_batch(ll_ctx *ctx, int first, int count, int enable);
/* The free function itself, on caller-supplied host correspondences (Corre_Match.src / .tgt, laserOdometry.cpp:165-172):
 * corner_case selects 5 regions instead of 10 (:179-188).  Outputs are per correspondence, in input order.          */
int ll_vote_host(ll_ctx *ctx, const ll_point *host_src, const ll_point *host_tgt, int n, int corner_case,
                 int *count, uint8_t *selected, float *weight);
/* per plane correspondence (in correspondence order): incompatibility count, selected flag, weight      */
int ll_download_vote(ll_ctx *ctx, int slot, int *count, uint8_t *selected, float *weight, int cap);

/* ---------------------------------------------------------------- a9-a10: residuals, Jacobians, GN
 * Residual blocks in Ceres order: n_edge LidarEdgeFactor blocks (3 rows, lidarFactor.hpp:9-52) then the
 * selected LidarPlaneFactor_modify blocks (1 row, :203-251, weight = vote weight), all with s = 1
 * (DISTORTION 0, laserOdometry.cpp:23).  pose: count x 7 doubles, NULL = the pose the ctx currently holds
 * for the slot (guess, or the result of the last ll_gn_step_batch).                                      */
int ll_normal_equations_batch(ll_ctx *ctx, int first, int count, const double *host_pose);
/* H: 36 doubles row-major over (dtheta[3], dt[3]) in the EigenQuaternionManifold tangent; g = J^T r; cost = sum rho/2 */
int ll_download_normal_equations(ll_ctx *ctx, int slot, double *H36, double *g6, double *cost);
/* Solve H d = -g (Cholesky, f64) on device, q <- Plus(q, d[0:3]), t += d[3:6]; one Gauss-Newton iteration.  */
int ll_gn_step_batch(ll_ctx *ctx, int first, int count);
int ll_download_pose(ll_ctx *ctx, int slot, double *pose7);
/* What ceres::CostFunction::Evaluate would return for the slot's blocks at `pose7`: residuals (rows),
 * jacobians[0] rows x 4 (ambient x,y,z,w) and jacobians[1] rows x 3, row-major; loss NOT applied
 * (Ceres applies it outside Evaluate).  rows = 3*n_edge + n_plane_selected.                             */
int ll_residual_jacobian(ll_ctx *ctx, int slot, const double *pose7, double *r, double *Jq, double *Jt, int cap_rows);

/* ---------------------------------------------------------------- the reference's solver and frame loop
 * ceres::Solve as laserOdometry.cpp:820-825 configures it: trust-region / Levenberg-Marquardt, DENSE_QR,
 * max_num_iterations = 4, every other option at its Ceres default.  ll_lm_default_options fills exactly those.       */
typedef struct {
    int    max_num_iterations;
    double initial_radius, max_radius, min_radius, min_relative_decrease, min_lm_diagonal, max_lm_diagonal;
    double function_tolerance, gradient_tolerance, parameter_tolerance;
    int    jacobi_scaling;
} ll_lm_options;
void ll_lm_default_options(ll_lm_options *o);
/* LM solve of the residual blocks the slot currently holds (after associate + vote), starting from the slot's pose;
 * the pose is replaced by the solution.  Device-resident, no host synchronisation; opt NULL = defaults.              */
int ll_lm_solve_batch(ll_ctx *ctx, int first, int count, const ll_lm_options *opt);
/* laserOdometry's per-frame body (:439-832) for the scans in slots [first, first+count), IN SEQUENCE: slot k's target
 * is slot k-1 (the carry for slot `first`), its initial para_q/para_t is the previous slot's result (host_pose0 for the
 * first; NULL = identity) -- the warm start of :61-65.  Per frame: n_outer (3, :439) x { associate, vote when the
 * frame's sequence index first_frame_index + k is > 5 (:794), LM solve }.  host_poses_out: count x 7, may be NULL.
 * The slots must have been extracted (ll_extract_batch).                                                             */
int ll_odometry_frames(ll_ctx *ctx, int first, int count, const double *host_pose0, int n_outer, int first_frame_index,
                       const ll_lm_options *opt, double *host_poses_out);
/* ---------------------------------------------------------------- TransformToEnd: the other half of motion compensation
 * With ll_params.distortion = 1 every point carries its interpolation ratio s, and TransformToStart slerps per point.  The reference's
 * TransformToEnd (laserOdometry.cpp:99-114) re-projects the clouds of the frame just solved to the END of its sweep -- the start of the
 * next one -- so that they can serve as the next frame's target and as laserMapping's input (:860-918); the reference calls it under
 * `if (0)` (:861) because KITTI arrives deskewed.  Per point p, with q = q_last_curr, t = t_last_curr as the solve left them (never
 * normalised):  un = Identity.slerp(s, q) * p + s * t  in f64, stored to f32 (the bits the association computes);
 * end = q.inverse() * (un - t)  in f64, stored to f32;  intensity = int(intensity).  Everything is rewritten IN PLACE:
 *   mode 1   the slot's less-sharp and less-flat clouds (what ll_set_target_from_slot, ll_associate_batch, the mapping frames and
 *            ll_download_features read afterwards);
 *   mode 2   also laserCloud (what ll_download_cloud and ll_drives_registered read).
 * A slot whose extraction was refused (status != 0) is left alone and is no error.
 *
 * ll_set_deskew switches it on for the frame loops (0 = off, the default: nothing the library computes changes by a bit).  With a
 * mode set, ll_odometry_frames deskews slot k with its solved pose after frame k's last outer iteration and rebuilds the slot's
 * search grids before frame k + 1 is associated; ll_odometry_sequences does the same per row for the row's running sequences (one
 * deskew and one grid launch more per row; a sequence that sits out keeps every byte of its clouds); ll_drives inherits it: the mapping
 * or localising frame of a step reads the deskewed clouds, and a lane's LL_DRIVE_START frame, which has no solve, is not deskewed.
 * The loops deskew only slots they solve -- the first target is whatever the caller set -- on the context's stream, without a host
 * synchronisation.  A non-finite solved pose makes non-finite clouds.  Checkpoints do not record the mode (as with
 * ll_drives_set_localize: set it again before ll_drives_restore); a saved carry holds the clouds as they are, and a restore into a
 * context whose mode is on marks the slots it fills as deskewed.  ll_hot_path_batch, ll_hot_path_chain and ll_associate_batch are NOT
 * affected: their pairs are independent by construction (every slot is solved from its own guess against a target nobody re-projects).
 * LL_ERR_ARG: mode outside 0..2; LL_ERR_STATE: the context has distortion = 0 -- there s = 1 and TransformToEnd is the identity up to
 * rounding: refused, not rounded.
 *
 * ll_deskew_slots is the stage on its own: slots [first, first + count) with host_pose7 ([count][7]; NULL = the poses the slots hold on
 * the device), mode 1 or 2, then their search grids anew.  No host synchronisation beyond the pose upload's.
 *
 * A slot is deskewed at most ONCE per extraction / upload -- a second application would transform again.  ll_extract_batch, the hot
 * path, ll_upload_scan* and ll_upload_features clear the mark of the slots they fill; ll_deskew_slots, and a loop asked to solve
 * such a slot while a mode is set, return LL_ERR_STATE before anything is enqueued, and ll_last_error names the slot.             */
int ll_set_deskew(ll_ctx *ctx, int mode);   /* 0 off (default); 1: less-sharp + less-flat; 2: also laserCloud */
int ll_deskew_slots(ll_ctx *ctx, int first, int count, const double *host_pose7 /* [count][7], NULL: the slots' device poses */, int mode /* 1 or 2 */);

/* The same frame loop for S independent sequences side by side: frame k of every sequence advances in one set of launches.
 * The frames live in a ring of rows, one row = S contiguous slots; frame row r of sequence q sits in slot
 *     base + (r mod ring_rows) * S + q,
 * and its target is the same sequence's frame at row r - 1 (modulo the ring).  Row row0 - 1 must hold every running
 * sequence's previous frame, extracted (for a fresh sequence its frame 0).  Rows row0 .. row0 + n_rows - 1 run:
 *   seq_rows[q]      rows sequence q runs in this call, 0..n_rows (NULL = n_rows for all); the slots of the rows it does
 *                    not run are not touched (no pose, pair header, correspondence or LM state is written),
 *   frame_index0[q]  the sequence's frame index of row row0: a frame votes when its index is > 5 (:794) (NULL = 1 for all),
 *   host_pose0       [S][7] warm start of row row0; NULL = the pose held by row row0 - 1's slot, which continues a drive
 *                    that streams through the ring: extract the next frames into the slots of finished rows, call again.
 * The warm start of row r + 1 is row r's solution (:61-65).  Everything is enqueued on the context stream; the call
 * synchronises only to fill host_poses_out ([n_rows][S][7], may be NULL; rows a sequence did not run are NaN).
 * LL_ERR_ARG (nothing enqueued): S < 1, ring_rows < 2, base < 0, base + S * ring_rows > batch, n_rows outside
 * 1..ring_rows - 1, seq_rows[q] outside 0..n_rows, n_outer outside 1..16, opt->max_num_iterations outside 0..64.   */
typedef struct {
    int base;        /* first slot of the ring */
    int n_seq;       /* S: sequences side by side */
    int ring_rows;   /* rows in the ring: slots [base, base + ring_rows * S) */
} ll_seq_layout;
int ll_odometry_sequences(ll_ctx *ctx, const ll_seq_layout *L, int row0, int n_rows, const int *seq_rows, const int *frame_index0,
                          const double *host_pose0, int n_outer, const ll_lm_options *opt, double *host_poses_out);

/* ---------------------------------------------------------------- laserMapping scan-to-submap (first stage)
 * The optimisation laserMapping runs per frame (laserMapping.cpp:1822-2095) for ONE scan against the corner / surf clouds
 * gathered from the cube map.  The cube bookkeeping (:1584-1808, :2101-2165) stays with the caller for now.
 * An ll_map shares the device and stream of the ll_ctx it was created from and must be destroyed before it.            */
typedef struct ll_map ll_map;
int  ll_map_create(ll_ctx *ctx, int max_map_corner, int max_map_surf, int max_scan_corner, int max_scan_surf, ll_map **out);
void ll_map_destroy(ll_map *m);
const char *ll_map_last_error(const ll_map *m);
/* kdtreeCornerFromMap->setInputCloud(laserCloudCornerFromMap) / kdtreeSurfFromMap (:1826-1827): upload + search grid */
int ll_map_set_map(ll_map *m, const ll_point *host_corner_from_map, int n_corner, const ll_point *host_surf_from_map, int n_surf);
/* laserCloudCornerStack / laserCloudSurfStack: the scan's (already down-sized, :1813-1821) feature clouds, sensor frame */
int ll_map_set_scan(ll_map *m, const ll_point *host_corner_stack, int n_corner, const ll_point *host_surf_stack, int n_surf);
/* One data-association pass (:1877-2047) at pose_w = parameters[7] (q_w_curr x,y,z,w, t_w_curr); NULL = the map's
 * current pose.  Produces the residual blocks in stack order: edges (stack index, point_a, point_b), planes (stack
 * index, unit norm, negative_OA_dot_norm).                                                                           */
int ll_map_associate(ll_map *m, const double *pose_w7);
int ll_map_get_counts(ll_map *m, int *n_edge, int *n_plane);
/* laserCloudCornerFromMap->points.size() / laserCloudSurfFromMap->points.size() (:1822: the block runs only above 10 / 50) */
int ll_map_get_map_sizes(ll_map *m, int *n_corner_from_map, int *n_surf_from_map);
int ll_map_download_edges(ll_map *m, int *src, double *a3, double *b3, int cap);
int ll_map_download_planes(ll_map *m, int *src, double *norm3, double *d, int cap);
/* H (6x6 row-major over the manifold tangent + t), g, cost of the current blocks at pose_w (NULL = current pose),
 * HuberLoss(0.1) + EigenQuaternionManifold as :1863-1866                                                            */
int ll_map_normal_equations(ll_map *m, const double *pose_w7, double *H36, double *g6, double *cost);
/* What ceres::CostFunction::Evaluate would return for the current blocks at pose_w (NULL = current pose): residuals,
 * jacobians[0] rows x 4 (ambient x,y,z,w), jacobians[1] rows x 3, row-major, loss NOT applied; rows = 3*n_edge + n_plane,
 * edges first -- for callers that keep ceres::Solve (:2073-2082) and only replace the data association.              */
int ll_map_residual_jacobian(ll_map *m, const double *pose_w7, double *r, double *Jq, double *Jt, int cap_rows);
/* The whole block :1822-2095: if the map holds > 10 corner and > 50 surf points, n_outer (2, :1832) x { associate,
 * ceres::Solve restated (LM, <= 4 iterations; opt NULL = ll_lm_default_options) }.  pose_w7 in/out; *ran = 0 when the
 * map is too small (the reference then keeps the odometry guess, :2096-2100).  LL_ERR_STATE: the solve left an
 * undefined (NaN) pose -- a lost hand-over inside the launch -- or the map holds a row / tile shard.                  */
int ll_map_optimize(ll_map *m, double *pose_w7, int n_outer, const ll_lm_options *opt, int *ran);

/* Row-parallel use over several GPUs (BASELINE config 4): every rank holds the same map and its share of the
 * stack points (ll_map_set_scan with a slice).  The residual blocks are independent, so the normal equations of the
 * whole scan are the SUM over ranks of ll_map_evaluate's 44-double record (H 36, g 6, cost, rows); the caller
 * all-reduces it (RCCL over xGMI: 28 unique doubles matter) and feeds the sum to ll_map_lm_begin / ll_map_lm_accept,
 * so that every rank advances an identical Levenberg-Marquardt state:
 *     associate;  evaluate -> all-reduce -> lm_begin;  repeat max_num_iterations x { lm_propose; evaluate -> all-reduce -> lm_accept }
 * ll_map_optimize is exactly this sequence on one rank without the all-reduce.                                          */
int ll_map_set_pose(ll_map *m, const double *pose_w7);
int ll_map_get_pose(ll_map *m, double *pose_w7);                                        /* LL_ERR_STATE: the pose on the device is undefined (NaN) */
int ll_map_evaluate(ll_map *m, double *neq44);                                           /* at the map's current pose */
int ll_map_lm_begin(ll_map *m, const double *neq44_sum, const ll_lm_options *opt);
int ll_map_lm_propose(ll_map *m, const ll_lm_options *opt);                               /* current pose <- candidate (or unchanged) */
int ll_map_lm_accept(ll_map *m, const double *neq44_sum, const ll_lm_options *opt);       /* current pose <- accepted state */

/* Tile-parallel use over several GPUs: the map -- not the scan -- is split; every rank holds the points
 * of ITS cubes (ll_cubemap_set_shard, or ll_map_set_map + ll_map_set_map_ids for a hand-made split) and the whole scan.
 *     repeat n_outer x { ll_map_knn_partial -> all-gather of the candidates -> ll_map_associate_merged -> ll_map_solve }
 * ll_map_knn_partial: the five nearest of this rank's points per stack point, nn = 5 x (x, y, z, squared distance) floats,
 * id = 5 global ids (INFINITY / INT_MAX in unused slots); buffers of n_stack * 5 entries, HOST OR DEVICE memory (the
 * all-gather is RCCL on device buffers over xGMI, 100 B per stack point and rank).  ll_map_associate_merged: the buffers
 * of all parts back to back ([part][stack point][5], host or device); keeps the five smallest (distance, id) -- the
 * global ids number the points in the order of the unsplit search cloud, so ties fall exactly as in ll_map_associate --
 * and runs the line / plane fit: every rank ends with the residual blocks ll_map_associate would give on the whole map.
 * ll_map_solve: one ceres::Solve restated on those blocks (replicated: <= a few thousand rows; identical on all ranks).
 * ll_map_set_map_ids: ids ascending in the order of the unsplit cloud; both NULL = back to positions.                  */
int ll_map_set_map_ids(ll_map *m, const int *corner_gid, const int *surf_gid);
int ll_map_knn_partial(ll_map *m, const double *pose_w7, float *corner_nn, int *corner_id, float *surf_nn, int *surf_id);
int ll_map_associate_merged(ll_map *m, const double *pose_w7, int n_parts, const float *corner_nn, const int *corner_id,
                            const float *surf_nn, const int *surf_id);
int ll_map_solve(ll_map *m, double *pose_w7, const ll_lm_options *opt);                 /* LL_ERR_STATE: row shard set, or an undefined (NaN) pose came out */
/* Device-resident variants of the same steps for the collectives: every pointer is a DEVICE pointer on the context's GPU, the
 * calls only enqueue on ll_stream(ctx) (no host hop, no synchronisation) and work at the pose already on the device
 * (ll_map_set_pose before, ll_map_get_pose after).  The caller's RCCL all-reduce (44 doubles, of which 28 matter) /
 * all-gather (100 B per stack point and rank) runs on the same buffers, stream-ordered with ll_stream(ctx); this is what
 * lightloam_amd/parallel.py does on the GPU box (laserMapping.cpp:1832-2095 spread over the GPUs of a node).              */
int ll_map_evaluate_dev(ll_map *m, double *neq44_dev);
int ll_map_lm_begin_dev(ll_map *m, const double *neq44_sum_dev, const ll_lm_options *opt);
int ll_map_lm_propose_dev(ll_map *m, const ll_lm_options *opt);
int ll_map_lm_accept_dev(ll_map *m, const double *neq44_sum_dev, const ll_lm_options *opt);
int ll_map_knn_partial_dev(ll_map *m, float *corner_nn_dev, int *corner_id_dev, float *surf_nn_dev, int *surf_id_dev);
int ll_map_associate_merged_dev(ll_map *m, int n_parts, const float *corner_nn_dev, const int *corner_id_dev,
                                const float *surf_nn_dev, const int *surf_id_dev);   /* buffers must stay valid until the stream has run it */
int ll_map_solve_dev(ll_map *m, const ll_lm_options *opt);
/* BASELINE config 4 in full -- tiles for the search AND rows for the solve: after ll_map_associate_merged every rank holds
 * all residual blocks; with a row shard set, ll_map_evaluate / ll_map_normal_equations sum only the blocks i with
 * i % world == rank, and the LM runs through evaluate -> all-reduce(JtJ, Jtr, cost) -> ll_map_lm_begin / _accept as in the
 * row-parallel scheme above (result within f64 summation-order rounding of one GPU; identical on all ranks).  (0, 1) =
 * all blocks.  ll_map_solve / ll_map_optimize refuse while a row shard is set.                                        */
int ll_map_set_row_shard(ll_map *m, int rank, int world);

/* ---------------------------------------------------------------- the graph-based correspondence vote in the mapping stage
 * Light-LOAM's vote, which the library has had in the odometry (a8, ll_vote_batch), on laserMapping's plane blocks.  The reference's
 * mapping stage is written for it -- laserMapping.cpp:1843-1850, :1993-2003, :2026 collect a Corre_Match per plane block that passed
 * the fit (src = the raw stack point, tgt = the float centroid of its five neighbours: float sums in K-NN order, :1960-1962, each
 * / 5 in float, :1969-1971), :836-1030 is mapping's own graph_based_correspondence_vote_simple, :2057-2072 feed the selected blocks
 * to the problem -- but the call is commented out.  It is opt-in here, off by default, and off changes nothing by a bit.
 *   The vote (:836-1030): 20 regions of n / 20 correspondences in stack order, the last one takes the remainder (n < 20: everything
 *   is in the last); every unordered pair of a region is incompatible, and counts for both, when
 *   (double)expf(-gap * gap) < 0.95 with gap = | |src_i - src_j| - |tgt_i - tgt_j| | on f32 square roots (0.95 is a double literal;
 *   bit-exact thresholds in csrc/ll_exact_math.h); an entry of a region of m is selected iff (float)count < 0.75f * (float)m
 *   (strict; corner_case = true at :2059).  The weight is 1: LidarPlaneNormFactor takes none.  Edge blocks are never voted.
 * Two decisions: (1) with the vote on, the plane blocks of the solve are the selected ones INSTEAD of all of them -- the intent of
 * the commented gate at :2027-2032; the literal text would add the selected blocks a second time on top of :2033.  (2) The selected
 * blocks keep stack order, as the odometry vote keeps correspondence order; the reference's order only permutes residual blocks.
 * What is not shown: no accuracy claim is made -- the synthetic drives have no outlier structure that would show one.
 * ll_map_set_vote(m, 1): ll_map_associate (at a host pose or, with NULL, at the device pose) and ll_map_optimize vote after the
 * compaction -- two launches more per association, no synchronisation; ll_map_get_counts, ll_map_download_planes and everything that
 * reads the blocks (normal equations, rows, solves) then see the selected blocks.  LL_ERR_STATE together with a row shard or a tile
 * shard (those modes stay un-voted; they in turn refuse while the vote is on); LL_ERR_ARG when a region of max_scan_surf / 20 + 19
 * candidates at 28 B each does not fit the 160 KiB of LDS.
 * ll_map_download_vote: the candidates of the last voted association, in stack order: stack index, count of incompatible pairs,
 * selected flag, tgt (3 floats each); any of the four may be NULL; *n = their number (cap < *n: LL_ERR_CAPACITY).
 * ll_map_vote_host: the same vote on caller-supplied correspondences through the same kernel (ll_vote_host's counterpart).          */
int ll_map_set_vote(ll_map *m, int on);
int ll_map_download_vote(ll_map *m, int *src, int *count, uint8_t *selected, float *tgt3, int cap, int *n);
int ll_map_vote_host(ll_ctx *ctx, const ll_point *src, const ll_point *tgt, int n, int *count, uint8_t *selected);

/* pcl::VoxelGrid<PointType>::filter on a whole cloud of any size (downSizeFilterCorner / downSizeFilterSurf,
 * laserMapping.cpp:1813-1821, :2151-2165): centroids (x, y, z, intensity) per voxel, in voxel-index order.       */
int ll_voxel_grid(ll_ctx *ctx, const ll_point *host_in, int n, float leaf_size, ll_point *host_out, int cap, int *n_out);

/* ---------------------------------------------------------------- lidarFactor.hpp functors on caller-supplied blocks
 * For a node that keeps its own association code and ceres::Problem and only wants the functors evaluated on the device
 * (include/lightloam_lidarFactor.hpp keeps LidarEdgeFactor::Create / LidarPlaneFactor_modify::Create /
 * LidarPlaneNormFactor::Create as they are called at laserOdometry.cpp:615, :783 and laserMapping.cpp:1918, :2033).
 * ll_factor_blocks_set: the blocks of one problem, f64 --
 *     edge9   [n_edge][9]   curr_point, last_point_a, last_point_b                         (lidarFactor.hpp:9-52,  3 rows each)
 *     plane13 [n_plane][13] curr_point, last_point_j, last_point_l, last_point_m, weight   (:203-251, 1 row each)
 *     pnorm7  [n_pnorm][7]  curr_point, plane_unit_norm, negative_OA_dot_norm              (:253-285, 1 row each)
 * all with s = 1 (what the reference's build passes: DISTORTION 0, laserOdometry.cpp:23, :81-84) unless ll_factor_blocks_set_s
 * follows: the functors' s_ of every edge / plane block (lidarFactor.hpp:25-27, :219-221: Identity.slerp(s, q), s * t), f64
 * [n_edge] and [n_plane]; NULL = all ones.  ll_factor_blocks_set resets them to one.
 * ll_factor_blocks_evaluate: residuals [rows], jacobians w.r.t. q (x, y, z, w) [rows][4] and t [rows][3], row-major,
 * rows = 3 n_edge + n_plane + n_pnorm in that order; loss functions are the caller's (Ceres applies them).         */
int ll_factor_blocks_set(ll_ctx *ctx, int n_edge, const double *edge9, int n_plane, const double *plane13, int n_pnorm, const double *pnorm7);
int ll_factor_blocks_set_s(ll_ctx *ctx, const double *edge_s, const double *plane_s);
int ll_factor_blocks_evaluate(ll_ctx *ctx, const double q[4], const double t[3], double *r, double *Jq, double *Jt, int cap_rows);

/* ---------------------------------------------------------------- laserMapping's cube map (second stage)
 * The 21 x 21 x 11 cubes of 50 m that hold the map (laserMapping.cpp:45-53, :74-75), resident in HBM, and the per-frame
 * body around the optimisation: ll_cubemap_prepare = :1584-1821 (centre cube of t_w_curr, the six shift loops, the
 * 5 x 5 x 3 valid cubes gathered into laserCloudCornerFromMap / SurfFromMap, the scan's less-sharp / less-flat clouds
 * down-sized to laserCloudCornerStack / SurfStack), ll_cubemap_optimize = :1822-2100, ll_cubemap_update = :2103-2165
 * (the registered scan's points into their cubes, every valid cube down-sized).  line_res / plane_res =
 * mapping_line_resolution / mapping_plane_resolution (:2363-2364, defaults 0.4 / 0.8).  pool_points: HBM points per
 * cloud type for the cubes (two pools of that size each).                                                          */
typedef struct ll_cubemap ll_cubemap;
int  ll_cubemap_create(ll_ctx *ctx, float line_res, float plane_res, int max_scan_corner, int max_scan_surf, int pool_points, ll_cubemap **out);
void ll_cubemap_destroy(ll_cubemap *cm);
const char *ll_cubemap_last_error(const ll_cubemap *cm);
int ll_cubemap_prepare(ll_cubemap *cm, const double *t_w3, const ll_point *host_corner_last, int n_corner, const ll_point *host_surf_last, int n_surf);
int ll_cubemap_optimize(ll_cubemap *cm, double *pose_w7, int n_outer, const ll_lm_options *opt, int *ran);
int ll_cubemap_update(ll_cubemap *cm, const double *pose_w7);
/* the three calls in sequence with the reference's constants; pose_w7 in: the guess of transformAssociateToMap (:1581) */
int ll_cubemap_process(ll_cubemap *cm, double *pose_w7, const ll_point *host_corner_last, int n_corner, const ll_point *host_surf_last, int n_surf, int *ran);
/* the same for the scan that sits in an extracted slot of the owning ll_ctx: its less-sharp / less-flat clouds go from the
 * slot to the map stage device-to-device (the laser_cloud_corner_last / laser_cloud_surf_last topics, laserOdometry.cpp:898-910) */
int ll_cubemap_process_slot(ll_cubemap *cm, double *pose_w7, int slot, int *ran);
/* Tile shard: this cube map keeps only the cubes owned by `rank` of `world` (ownership is a function of the cube's
 * position in the world, so the shift loops never move a cube between ranks); call before the first scan.  prepare and
 * update work as before on the owned cubes (prepare also numbers the gathered points for ll_map_knn_partial);
 * ll_cubemap_optimize / _process refuse (LL_ERR_STATE): the search goes through ll_cubemap_map() and the calls above.
 * The union of the ranks' cubes is the unsplit cube map, cube by cube and bit for bit.                               */
int ll_cubemap_set_shard(ll_cubemap *cm, int rank, int world);
ll_map *ll_cubemap_map(ll_cubemap *cm);                       /* the inner ll_map (owned by the cube map) */
int ll_cubemap_set_vote(ll_cubemap *cm, int on);               /* ll_map_set_vote of the inner map: ll_cubemap_optimize / _process* then vote */
/* cen3: laserCloudCenWidth / Height / Depth; counts4: corner / surf from map, corner / surf stack */
int ll_cubemap_info(ll_cubemap *cm, int *cen3, int *counts4);
/* which: 0 laserCloudCornerFromMap, 1 laserCloudSurfFromMap, 2 laserCloudCornerStack, 3 laserCloudSurfStack */
int ll_cubemap_download_cloud(ll_cubemap *cm, int which, ll_point *out, int cap, int *n);
int ll_cubemap_download_cube(ll_cubemap *cm, int surf, int cube_index, ll_point *out, int cap, int *n);

/* ---------------------------------------------------------------- laserMapping's cube map for many sequences side by side
 * S independent cube maps, each what an ll_cubemap created with the same parameters holds.  One call runs one frame of
 * :1584-2165 for every running sequence in one set of launches per stage; the host synchronises five times per frame (the
 * slots' headers -- not for host clouds --, prepare, the poses, the per-cube counts, the filtered sizes), plus one per voxel-filter or by-cube sort
 * that is too large to stay inside its workgroups (clouds of more than 65 536 points), whatever S is.
 * Contract: sequence q after any number of calls equals an ll_cubemap driven by ll_cubemap_process_slot / _process with
 * the same frames, bit for bit: pose, ran, cen, the four clouds, every cube.  Tile and row shards are not supported.
 * ll_cubemaps_process_slots: the scan of sequence q is the extracted slot slots[q] of the owning context (device to
 * device); slots[q] = -1: sequence q does not run this frame -- its map, its pose_w7 row and ran[q] are not touched.
 * pose_w7 [S][7]: in = the guess of transformAssociateToMap (:1581), out = the optimised parameters[]; ran [S] may be NULL.
 * ll_cubemaps_process: the same from host clouds; a sequence whose two cloud pointers are NULL does not run.
 * Errors: LL_ERR_ARG before anything is enqueued (n_seq < 1, a slot out of range, a slot used by two sequences, bad
 * clouds); LL_ERR_STATE for a slot that holds no extracted scan, or a solve that leaves a NaN pose (last_error names the
 * sequence); LL_ERR_CAPACITY when a pool would overflow -- decided for every sequence and both cloud types before any
 * pair table changes, so no cube changes in that call and the call can be repeated.
 * ll_cubemaps_stats: host synchronisations and frames since create.                                                 */
typedef struct ll_cubemaps ll_cubemaps;
int  ll_cubemaps_create(ll_ctx *ctx, int n_seq, float line_res, float plane_res, int max_scan_corner, int max_scan_surf, int pool_points, ll_cubemaps **out);
void ll_cubemaps_destroy(ll_cubemaps *cms);
const char *ll_cubemaps_last_error(const ll_cubemaps *cms);
int  ll_cubemaps_process_slots(ll_cubemaps *cms, const int *slots, double *pose_w7, int *ran);
int  ll_cubemaps_process(ll_cubemaps *cms, const ll_point *const *corner_last, const int *n_corner, const ll_point *const *surf_last,
                         const int *n_surf, double *pose_w7, int *ran);
int  ll_cubemaps_info(ll_cubemaps *cms, int q, int *cen3, int *counts4);
int  ll_cubemaps_download_cloud(ll_cubemaps *cms, int q, int which, ll_point *out, int cap, int *n);
int  ll_cubemaps_download_cube(ll_cubemaps *cms, int q, int surf, int cube_index, ll_point *out, int cap, int *n);
int  ll_cubemaps_stats(const ll_cubemaps *cms, long long *syncs, long long *frames);
/* The mapping vote (ll_map_set_vote) per sequence: on[q] = 1 votes sequence q's plane blocks in ll_cubemaps_process* from now on, until
 * changed -- two launches more per outer iteration of a frame in which any sequence votes, no synchronisation more.
 * ll_cubemaps_localize_slots never votes: its fit record keeps its meaning.                                          */
int  ll_cubemaps_set_vote(ll_cubemaps *cms, const int *on /* [n_seq] */);
/* sequence q back to what ll_cubemaps_create gave it (centre, counts, pool cursors, pair tables); the others are untouched */
int  ll_cubemaps_reset(ll_cubemaps *cms, int q);

/* ---------------------------------------------------------------- map export: laserCloudSurround and laserCloudMap
 * laserMapping's two map publications -- the surround cloud every 5th frame (laserMapping.cpp:2173-2188) and the whole map
 * every 20th (:2190-2203) -- for any subset of the S sequences in one call: the host lists the selected clouds from its pair
 * tables, ONE gather kernel packs them on the device, ONE copy brings them to `out`, and the host synchronises ONCE, whatever
 * S and the number of cubes are.  which [S] selects per sequence what it contributes; `out` may be host memory (pageable or
 * page-locked) or device memory (the gather then writes to it directly).
 * Order: the sequences back to back in sequence order; inside one sequence the cubes in list order (LL_MAP_SURROUND: the i, j,
 * k loop order of :1784-1801; LL_MAP_ALL: cube index 0 .. 4850), per cube the corner cloud, then the surf cloud, each in the
 * cube's own point order -- the concatenation of ll_cubemaps_download_cube(q, 0, c), (q, 1, c) over the list, byte for byte.
 * Surround set: the valid cubes of the last frame that sequence ran, read after that frame's update, as in the reference (the
 * list is made at :1784-1801, the cubes are read at :2176-2181, after the filters of :2150-2168).  A sequence that has not
 * run a frame since create or ll_cubemaps_reset exports 0 points in either mode.
 * Read-only: an export changes no pool, pair table, pose or counter of the maps other than ll_cubemaps_stats' syncs; it may be
 * called between any two frames, and through ll_drives_cubemaps(d) between any two ll_drives_step calls.
 * Host synchronisations: ll_cubemaps_export / ll_cubemap_export exactly one per successful call (added to syncs; the first
 * calls also allocate the device staging buffer, which grows to the need and never beyond the pools' live points);
 * ll_cubemaps_export_sizes none -- it is host bookkeeping, with no launch.
 * offset [S + 1]: sequence q's points are out[offset[q] .. offset[q + 1]); totals are long long (128 maps can pass 2^31 bytes).
 * Errors: LL_ERR_ARG before anything is enqueued (NULL handle / which, a value outside -1 .. 1, negative cap, out == NULL with
 * a non-zero total); LL_ERR_CAPACITY when the total exceeds cap -- offset is still filled, out is not touched, nothing is
 * launched; LL_ERR_STATE when a SELECTED sequence's map is unusable (an update failed half-way; last_error names it) -- one
 * that is not selected does not stop the others; LL_ERR_HIP when the staging buffer cannot be allocated (last_error has the
 * size; the object stays usable).  A tile-sharded single map (ll_cubemap_set_shard) exports the cubes it owns.
 * ll_cubemaps_export_timing: the last export's table build (host clock), gather and copy (device events) in ms, and its
 * points, segments (non-empty clouds) and tiles (workgroups of the gather); either pointer may be NULL.               */
#define LL_MAP_NONE     (-1)   /* the sequence is left out */
#define LL_MAP_SURROUND   0    /* the cubes of laserCloudSurroundInd of the sequence's last frame (:1784-1801), as :2175-2181 adds them */
#define LL_MAP_ALL        1    /* all 4851 cubes, as :2192-2197 adds them */
int  ll_cubemaps_export_sizes(ll_cubemaps *cms, const int *which /* [S] */, long long *offset /* [S + 1] */);
int  ll_cubemaps_export(ll_cubemaps *cms, const int *which /* [S] */, ll_point *out, long long cap, long long *offset /* [S + 1], may be NULL */);
int  ll_cubemaps_export_timing(const ll_cubemaps *cms, double *ms3, long long *counts3);
/* the same for the single cube map (the ROS node's map); n (may be NULL): the points of the selection, also on LL_ERR_CAPACITY */
int  ll_cubemap_export(ll_cubemap *cm, int which, ll_point *out, long long cap, long long *n);

/* ---------------------------------------------------------------- map import: the export's inverse
 * ll_cubemaps_layout (host bookkeeping: no launch, no synchronisation) gives what an LL_MAP_ALL export does not say about map q:
 * the centre cen3, the per-cube point counts counts [2][4851] (corner, then surf), and the valid list of the last frame
 * (valid [125], *n_valid entries) that LL_MAP_SURROUND reads.  Together with the LL_MAP_ALL cloud this is the complete state
 * of the map; where the clouds lie inside the pools is not part of it (nothing reads a pool except through its tables).
 * Any out pointer may be NULL.  LL_ERR_STATE for an unusable map.
 * ll_cubemaps_import puts such state back.  `points` is exactly the byte layout ll_cubemaps_export(.., LL_MAP_ALL) writes --
 * the sequences back to back (sequence q at points[offset[q] .. offset[q + 1])), cubes 0 .. 4850, per cube the corner cloud,
 * then the surf cloud -- in host memory (pageable or page-locked) or in device memory.  sel [S] (0 / 1) selects the sequences to
 * load; cen3 [S][3], counts [S][2][4851], valid [S][125] and n_valid [S] are read for the selected ones only.  For any S and
 * any number of cubes: ONE upload of the points (none when they are on the device), one table upload, ONE scatter kernel and
 * ONE host synchronisation, added to ll_cubemaps_stats' syncs.
 * A selected map is replaced whole, as if ll_cubemaps_reset had run first (ll_cubemaps_info's four cloud sizes are 0 until its
 * next frame); its pools end compact, in cube order.  A map that is not selected is untouched.
 * Errors, all decided before anything is enqueued or any table changes: LL_ERR_ARG for a NULL pointer, a sel outside 0 / 1,
 * an offset that is not ascending, counts that do not add up to the sequence's share of offset, a negative count, a centre
 * beyond +-2^24 (the centre is the array index of the world's origin cube and legitimately leaves 0 .. 20 on any long drive,
 * so only values the cube arithmetic cannot hold are refused), n_valid outside 0 .. 125 or a valid entry outside 0 .. 4850 or
 * listed twice; LL_ERR_CAPACITY when one type's points exceed pool_points (last_error names the sequence); LL_ERR_HIP when
 * the staging buffer cannot be allocated (the object stays usable).
 * ll_cubemap_layout / ll_cubemap_import: the same for the single map (n: the points of the cloud); a tile-sharded map accepts
 * only counts in cubes it owns (LL_ERR_ARG otherwise).                                                                       */
int  ll_cubemaps_layout(ll_cubemaps *cms, int q, int *cen3, int *counts /* [2][4851] */, int *valid /* [125] */, int *n_valid);
int  ll_cubemaps_import(ll_cubemaps *cms, const int *sel /* [S] */, const ll_point *points, const long long *offset /* [S + 1] */,
                        const int *cen3 /* [S][3] */, const int *counts /* [S][2][4851] */, const int *valid /* [S][125] */, const int *n_valid /* [S] */);
int  ll_cubemap_layout(ll_cubemap *cm, int *cen3, int *counts, int *valid, int *n_valid);
int  ll_cubemap_import(ll_cubemap *cm, const ll_point *points, long long n, const int *cen3, const int *counts, const int *valid, int n_valid);

/* ---------------------------------------------------------------- map merge: cube maps combined under a rigid transform
 * One merge op (dst, src, T): dst and src are two different maps of one ll_cubemaps; T (pose_w7 layout: qx, qy, qz, qw, tx, ty,
 * tz) takes src's world frame into dst's and is used as given -- pointAssociateToMap never normalises (laserMapping.cpp:125-134).
 * Per cloud type (0 corner, 1 surf), independently:
 *   order      src's points in the order ll_cubemaps_export(.., LL_MAP_ALL) lists that type: cube 0 .. 4850, inside a cube its own
 *              point order;
 *   transform  pointAssociateToMap (:125-134) in f64, the translation added last, rounded to float once per coordinate; the
 *              fourth float is carried over.  With the identity T every coordinate keeps its bits;
 *   binning    the cube arithmetic of :2108-2125 with dst's centre, the negative-side decrement included; a point whose cube lies
 *              outside 0..20 x 0..20 x 0..10 is dropped and counted;
 *   touched    a dst cube that receives at least one point becomes its old cloud followed by the new points in that order, passed
 *              through the library's VoxelGrid (:2151-2165) with the type's leaf (line_res / plane_res).  EVERY touched cube is
 *              filtered, not only those of dst's valid list: a merge has no current frame.
 * A cube that receives nothing is unchanged byte for byte; dst's centre, valid list and four per-frame clouds
 * (ll_cubemaps_download_cloud) are unchanged; src is unchanged whole.  added[i][w]: the points of op i, type w that entered a
 * cube (before the filter); dropped[i][w]: those that fell outside the array.  Either may be NULL.
 * Nothing passes through the host: the points are read where they lie in src's pool, ordered by destination cube by a counting
 * sort that is stable and gives the same bytes on every run, gathered behind the touched cubes' old clouds, filtered in one
 * VoxelGrid call per type over all ops, and copied into dst's pool in one launch.  The workspace grows to the need of the call
 * and is freed with the object.  Host synchronisations per successful call, whatever n_ops is: THREE (the per-cube counts, the
 * filtered sizes, the commit), plus one per cloud type whose filter call is above 65 536 points with a cube above 8 192 points (or
 * one cube only) -- the voxel filter's documented read-back; all are added to ll_cubemaps_stats' syncs.  frames does not rise.
 * The handle from ll_drives_cubemaps(d) is accepted between any two ll_drives_step calls; a lane that localises against dst
 * (ll_drives_set_localize) sees the merged map from its next step.
 * Errors: LL_ERR_ARG, decided before anything is enqueued: NULL handle or ops, n_ops < 1, a map index out of range, dst == src, a
 * map that is dst of two ops, a map that is dst of one op and src of another (a map may be src of several ops), a non-finite T.
 * LL_ERR_STATE, also before anything is enqueued: a dst or src map that is unusable (last_error names it).  LL_ERR_CAPACITY,
 * decided for every op and both types from the per-cube counts, before any pair table changes: a dst pool cannot hold what the map
 * holds of one type plus that type's added points (last_error names the op and the type) -- no cube of any map has changed and the
 * call can be repeated on an object with a larger pool_points.  LL_ERR_HIP: the workspace cannot be allocated (the object
 * stays usable) or a runtime call failed.
 * ll_cubemaps_merge_timing: the last merge's device time per stage in ms (assign, sort + gather, filter, commit; events) and its
 * counts (source points, touched cubes, points written to the pools); either pointer may be NULL.                            */
typedef struct { int dst, src; double T_w7[7]; } ll_merge_op;
int  ll_cubemaps_merge(ll_cubemaps *cms, const ll_merge_op *ops, int n_ops,
                       long long *added /* [n_ops][2], may be NULL */, long long *dropped /* [n_ops][2], may be NULL */);
int  ll_cubemaps_merge_timing(const ll_cubemaps *cms, double *ms /* assign, sort+gather, filter, commit */, long long *counts /* points in, touched cubes, points out */);

/* ---------------------------------------------------------------- whole drives side by side
 * S lanes; each runs one drive at a time through registration (ll_extract_batch), odometry (ll_odometry_sequences, one
 * row) and mapping (ll_cubemaps), the single-drive chain of ll_odometry_kitti with mapping = 1 for every lane at once.
 * The object uses slots [base, base + 2 S) of the context as two rows of S: one step reads lane q's raw scan from
 * ll_drives_slots()[q] (upload it there first, with any upload entry point), and advances every running lane by one frame:
 *   LL_DRIVE_IDLE   the lane does nothing; a drive ends when its lane goes idle
 *   LL_DRIVE_RUN    the next frame of the lane's drive; only after a step on which the lane ran, or a restore (lane checkpoints, below)
 *   LL_DRIVE_START  frame 0 of a new drive: a fresh cube map (ll_cubemaps_reset), identity world-odometry and map-to-odom
 *                   poses; pose0[q] (NULL: identity) is the odometry warm start of the drive's frame 1
 * Per step: extract over the row, odometry of the RUN lanes (frame index counted per lane, frame 1 = first odometry frame),
 * then on the device the world pose (laserOdometry.cpp:830-831), transformAssociateToMap (laserMapping.cpp:113-117), the
 * mapping frame (:1584-2165) and transformUpdate (:119-123).  The host synchronises only where the cube-map frame does.
 * This is a batch runner: every frame is mapped (laserMapping.cpp:1572-1576 drops buffered frames to keep real time).
 * Outputs ([S][7] / [S], each may be NULL; rows of lanes that did not run are NaN / 0):
 *   odom_w7    laserOdometry's q_w_curr, t_w_curr;   mapped_w7   laserMapping's parameters[] after the frame;
 *   ran        as ll_cubemaps_process_slots gives it.
 * Lane q equals, bit for bit, its drive run alone through ll_odometry_frames, WorldPose and an ll_cubemap.
 * keep_registered = 1: each step also keeps every running lane's full-resolution scan moved into the map frame
 * (/velodyne_cloud_registered, :2203-2213), in laserCloud order; ll_drives_registered copies one lane's out.
 * Errors: LL_ERR_ARG before anything is enqueued (a cmd outside 0..2, RUN on a lane that did not run on the previous step,
 * a non-finite pose0 row of a START lane; at create: base + 2 S beyond the batch, n_outer outside 1..16).  LL_ERR_STATE
 * for a scan the registration refused (status other than OK / EMPTY), LL_ERR_CAPACITY / LL_ERR_STATE from the mapping
 * stage: the step is lost for every lane that ran, and those lanes are stopped -- their next command must be IDLE or
 * START.  last_error names the lane at fault.  There is no retry protocol.
 * ll_drives_stats: host synchronisations inside steps, and steps that ran at least one lane.                          */
typedef struct ll_drives ll_drives;
typedef struct {
    int   n_lanes;                          /* S */
    int   base;                             /* the object uses slots [base, base + 2 S) of the context */
    float line_res, plane_res;              /* as ll_cubemaps_create (0.4, 0.8) */
    int   max_scan_corner, max_scan_surf, pool_points;
    int   n_outer;                          /* odometry outer iterations, 1..16 (3) */
    int   keep_registered;                  /* 1: each step keeps every running lane's registered full-resolution cloud */
} ll_drives_params;
#define LL_DRIVE_IDLE  0
#define LL_DRIVE_RUN   1
#define LL_DRIVE_START 2
int  ll_drives_create(ll_ctx *ctx, const ll_drives_params *p, ll_drives **out);
void ll_drives_destroy(ll_drives *d);
const char *ll_drives_last_error(const ll_drives *d);
int  ll_drives_slots(ll_drives *d, int *slots);   /* [S]: the slot the next step reads lane q's raw scan from */
int  ll_drives_step(ll_drives *d, const int *cmd, const double *pose0, double *odom_w7, double *mapped_w7, int *ran);
int  ll_drives_registered(ll_drives *d, int lane, ll_point *out, int cap, int *n);   /* the last step's cloud of that lane (n = 0: it did not run) */
int  ll_drives_stats(const ll_drives *d, long long *syncs, long long *frames);
ll_cubemaps *ll_drives_cubemaps(ll_drives *d);    /* borrowed: info / cloud / cube of each lane's map */
/* The mapping vote (ll_map_set_vote) in the lanes that map: a lane votes in the frames whose per-lane frame index (0 at START) is
 * > from_frame -- the reference's gate is 20 (:2057) -- negative = off, the default.  Localising lanes never vote.  The setting is not
 * part of a checkpoint (the blob format is unchanged): set it again after ll_drives_restore.  While it is >= 0 every step sets the
 * lanes' switches itself; with it off they are left as ll_cubemaps_set_vote on ll_drives_cubemaps(d) put them.                     */
int ll_drives_set_map_vote(ll_drives *d, int from_frame);

/* ---------------------------------------------------------------- lane checkpoints
 * A lane's state between two steps is its cube map (ll_cubemaps_layout + the LL_MAP_ALL cloud), its world-odometry and
 * map-to-odom poses, its frame counter (the vote switches on at frame 6) and the previous row's slot: the four feature clouds
 * and the solved pose, the target and the warm start of the lane's next odometry frame.  ll_drives_save writes that for the
 * selected lanes (lanes [S], 0 / 1) into one self-describing blob (INTEGRATION.md documents the format); ll_drives_restore
 * puts record r of a blob into lane into[r] (-1: the record is skipped) of this object -- another lane index, another
 * ll_drives with another S and base, a fresh context, another process.  The restored lane counts as having run: its next
 * command may be RUN (the drive continues, bit for bit as if it had never stopped), IDLE or START.
 * ll_drives_save_size: the blob's bytes, from host bookkeeping (no launch, no synchronisation); a negative value is an error code.
 * ll_drives_save: ONE pack launch (the export gather's tiles, the ring-strided less-flat cloud closed up in
 * ll_download_features' order, the poses and the counter), ONE copy and ONE synchronisation whatever the selection; `blob` may
 * be host memory or (16-byte aligned) device memory; *bytes (may be NULL) is filled whenever the selection is valid.  The call
 * is read-only: the run continues exactly as if it had not saved, apart from the syncs counters (ll_drives_stats and
 * ll_cubemaps_stats rise by one).  A lane can be saved when it ran on the previous step, or was restored and has not stepped
 * since; LL_ERR_STATE otherwise.  LL_ERR_CAPACITY when cap is too small: blob is not touched.  The pack launch checks every
 * ring-strided less-flat cloud against the size in its scan header; a mismatch is LL_ERR_STATE and the blob gets no header.
 * ll_drives_restore (blob in host memory): ONE upload, one import scatter, one small state kernel, the search grids of the
 * restored slots as ll_upload_features builds them (one launch per run of neighbouring lanes: one when all lanes or a
 * contiguous block are restored) and ONE synchronisation.  The lane's previous-row slot receives the
 * feature clouds the way ll_upload_features leaves a slot.  Every refusal is made before any lane changes: LL_ERR_ARG (last_error names the
 * field) for a wrong magic or version, a truncated or inconsistent blob, n_scans, distortion, line_res or plane_res that differ
 * from the destination's, an into entry that is no lane, two records into one lane; LL_ERR_CAPACITY when pool_points or a
 * per-scan feature capacity of the destination is too small.
 * ll_checkpoint_describe: pure host code, no device and no context: validates a blob and returns its header fields and, in
 * info->records (caller's array of info->cap_records entries, may be NULL), the per-record sizes.  LL_ERR_ARG as above.    */
typedef struct {
    int       lane;                          /* the lane the record was saved from */
    int       frame_index;                   /* of the lane's last frame (0: only frame 0 has run) */
    long long n_corner, n_surf;              /* map points per type */
    int       n_features[4];                 /* sharp, less sharp, flat, less flat of the previous-row slot */
    long long offset, bytes;                 /* the record's device payload inside the blob */
} ll_checkpoint_record;
typedef struct {
    int       version, n_records;
    long long total_bytes;
    int       n_scans, distortion, voxel_sort_ranks;
    float     line_res, plane_res;
    int       need_features[4];              /* the per-scan feature capacities a destination needs */
    ll_checkpoint_record *records;           /* in: the caller's array or NULL */
    int       cap_records;                   /* in: its entries */
} ll_checkpoint_info;
long long ll_drives_save_size(ll_drives *d, const int *lanes /* [S] */);
int  ll_drives_save(ll_drives *d, const int *lanes /* [S] */, void *blob, long long cap, long long *bytes);
int  ll_drives_restore(ll_drives *d, const int *into /* [records] */, const void *blob, long long bytes);
int  ll_checkpoint_describe(const void *blob, long long bytes, ll_checkpoint_info *info);

/* ---------------------------------------------------------------- localisation against frozen cube maps
 * ll_cubemaps_localize_slots: one READ-ONLY frame for every running sequence, :1584-1593, :1783-1821 and :1822-2100 without
 * the update (:2103-2165): poses in a map's frame while no pool, pair table, cen, valid list, broken flag or frame counter of
 * any map changes (map m's LL_MAP_SURROUND set stays that of the last frame that mapped into it).  Conventions are those of
 * ll_cubemaps_process_slots: slots[q] = -1: sequence q sits out, its pose_w7, ran and fit rows are not touched; otherwise it
 * reads the extracted slot slots[q] and localises against map map_of[q] (NULL: its own map q), any of the S maps, which several
 * sequences may share; its workspace (search clouds, stacks, grids: what ll_cubemaps_download_cloud(q, ..) shows) is its own.
 * map_of entries of sequences that sit out are not read.
 * No shift loops (:1595-1781): a shared map cannot be re-indexed for one reader.  The centre cube comes from the guess's
 * translation and the map's cen as in a mapping frame; the cubes i +-2, j +-2, k +-1 around it that lie inside the 21 x 21 x 11
 * array are gathered in that loop order, a cube outside the array holds nothing.  CONDITION: this equals, cloud for cloud and
 * bit for bit, a private copy of the map that runs the shift loops as long as that copy's shifts push no non-empty cube off
 * the array (a shift only translates indices and brings in empty cubes).  Where a private copy would have shifted occupied
 * cubes away, laserMapping forgets them and this call still reads those of them that lie inside the array.
 * Then per sequence the :1813-1821 filters, the search grids and 2 x {knn, compact, LM} under the :1822 gate; ran as today.
 * fit (may be NULL: then neither of the following is launched): for every sequence that optimised, one more association pass
 * at the final pose and one reduction kernel fill
 *   n_edge, n_plane     the residual blocks there, as ll_map_get_counts after ll_map_associate(final pose)
 *   cost                ll_map_normal_equations' cost there (HuberLoss(0.1))
 *   sq_edge, sq_plane   the sums of squares of ll_map_residual_jacobian's residuals there, loss not applied: the 3 n_edge edge
 *                       rows, the n_plane plane rows
 * and zeros for a running sequence that did not optimise.  sqrt(sq_plane / n_plane) is the RMS point-to-plane distance in
 * metres; a vehicle that leaves the map shows falling counts and, at the edge of the array, ran = 0.
 * Host synchronisations: three per call whatever S is (the slots' headers, prepare, poses + fit in one copy), plus the voxel
 * filter's read-back for clouds above 65 536 points; added to ll_cubemaps_stats' syncs.  frames does not rise.
 * Errors, all decided before any kernel is enqueued: LL_ERR_ARG (NULL handle, slots or pose; a slot out of range or used twice; a
 * map_of entry outside 0..S-1); LL_ERR_STATE (a selected slot without an extracted scan; a read map that is broken);
 * LL_ERR_CAPACITY (a scan larger than the create-time capacity; gathered cubes larger than the reader's search-cloud capacity).
 * LL_ERR_STATE also for a NaN pose out of a solve (last_error names the sequence).  A failed call changes no map.
 *
 * ll_drives_set_localize: map_of[q] = -1: lane q maps into its own map (the state after create); m >= 0: lane q localises
 * against lane m's map.  The mode holds until the next call and may change between any two steps, also for a running lane.  For
 * a localising lane LL_DRIVE_START resets no map: world-odometry = identity, map-to-odom (q_wmap_wodom, t_wmap_wodom) =
 * start_w7[q] (NULL: identity), where the drive begins in the map; LL_DRIVE_RUN is odometry, the world pose and
 * transformAssociateToMap as ever, then the read-only frame above instead of the mapping frame, then transformUpdate on the
 * localised pose.  mapped_w7 is the localised pose; odom_w7, ran and keep_registered (the cloud lands in the map's frame) as
 * for mapping lanes.  One step may hold both kinds: at most 5 (mapping lanes) + 3 (localising lanes) synchronisations, plus
 * filter read-backs, whatever S is.  The call itself uploads start_w7 and synchronises once (not counted: it is outside a step).
 * A step that would write a map another running lane reads -- cmd[m] != IDLE with map_of[m] = -1 while a running lane q != m
 * has map_of[q] = m -- is LL_ERR_ARG before anything is enqueued; last_error names both lanes.  LL_ERR_ARG also for a map_of
 * entry outside -1..S-1 or a non-finite start row of a localising lane.
 * A lane's mode is not part of a checkpoint: a restored lane continues in the mode ll_drives_set_localize gives it.
 * ll_drives_fit: the last step's records [S]; zeros for lanes that mapped, sat out or did not optimise.                    */
typedef struct { int n_edge, n_plane; double cost, sq_edge, sq_plane; } ll_localize_fit;
int  ll_cubemaps_localize_slots(ll_cubemaps *cms, const int *slots /* [S] */, const int *map_of /* [S], NULL: own map */,
                                double *pose_w7 /* [S][7] */, int *ran /* [S], may be NULL */, ll_localize_fit *fit /* [S], may be NULL */);
int  ll_drives_set_localize(ll_drives *d, const int *map_of /* [S] */, const double *start_w7 /* [S][7], may be NULL */);
int  ll_drives_fit(ll_drives *d, ll_localize_fit *fit /* [S] */);

/* ---------------------------------------------------------------- one cube map registered to another
 * ll_cubemaps_align: op i = (dst, src, T0_w7), in ll_merge_op's layout, estimates the rigid transform that takes map src's world
 * frame into map dst's: the T a following ll_cubemaps_merge needs.  It is laserMapping's scan-to-map optimisation (:1822-2095)
 * over the WHOLE of both maps, started at T0 (used as given, never normalised) -- local registration from a guess inside the
 * basin of the 1 m association radius, not global relocalisation.  Per cloud type w (0 corner, 1 surf) MAP_w = dst's points of the
 * type in the order an LL_MAP_ALL export lists them (cube index ascending, own order inside a cube) and STK_w = src's in the same
 * order; the result is what ll_map_optimize gives for the search clouds MAP_0, MAP_1, the scan STK_0, STK_1 (no voxel filter of
 * the stacks: a map's cubes are filtered at the stacks' leaf sizes already), the pose T0 and the same n_outer and opt:
 *   gate     :1822 (more than 10 corner and more than 50 surf points in dst); shut: ran[i] = 0, T comes back as given, fit all zero;
 *   n_outer x { pointAssociateToMap of every stack point; its exact five nearest in MAP_w by (distance, index in MAP_w); the
 *              nb == 5 && bd[4] < 1 acceptance; line / plane fit; ceres::Solve with `opt` (NULL: ll_lm_default_options) }
 *   fit      != NULL: the residual blocks once more at the final T and ll_localize_fit's five figures with the meaning they have
 *              there; NULL: that pass is not launched, the poses are the same bits.
 * n_outer = 0 is allowed: no solve, T comes back as given, ran reports the gate, the record describes the blocks at T0 -- how a
 * caller scores a transform it already has.
 * Read-only: no pool, pair table, centre, valid list, per-frame cloud or counter of any map changes (ll_cubemaps_stats' syncs
 * rises); a map may be dst and src of any number of ops.  Each op's T, ran and fit are the same bits whether it runs alone or among
 * others, and from call to call.
 * Nothing passes through the host.  Per distinct dst map and type the call builds a search structure over the whole map: occupied
 * cube -> slot, per slot 40^3 + 1 ints over world-anchored cells of 1.25 m (256 KB per occupied cube and type), the points in (cube,
 * cell) order; the normal equations are summed over (op, chunk of 1024 blocks) workgroups and one small workgroup per op takes the
 * Levenberg-Marquardt steps, n_outer x (1 + max_num_iterations) launch pairs enqueued back to back.  The search is exact for maps
 * whose points lie in the cubes the library's own arithmetic gives them (every frame, merge, and import of an export).  The
 * workspace grows to the need of the call and is freed with the object.
 * Host synchronisations per call in which an op passes the gate, whatever n_ops, n_outer, the maps' sizes and fit are: ONE (poses,
 * records and block counts in one copy); none otherwise.  Added to ll_cubemaps_stats' syncs; frames does not rise.
 * The handle from ll_drives_cubemaps(d) is accepted between any two ll_drives_step calls.
 * Errors, decided before anything is enqueued, last_error names the op: LL_ERR_ARG for a NULL handle, n_ops < 0, n_outer < 0, ops or
 * T_w7 NULL with n_ops > 0, a map index out of range, dst == src; LL_ERR_STATE for an unusable map or a NaN in T0; LL_ERR_CAPACITY
 * above 2^30 map or stack points.  LL_ERR_STATE also when a solve returns a NaN pose (cms_optimize's rule; the other ops' results are
 * delivered).  LL_ERR_HIP: the workspace cannot be allocated (the object stays usable) or a runtime call failed.
 * ll_cubemaps_align_timing: the last call's device time per stage in ms (build, search + fit, evaluate + solve, fit record; events)
 * and its counts (stack points, map points, residual blocks at the end, summed over the ops that ran); either may be NULL.        */
int  ll_cubemaps_align(ll_cubemaps *cms, const ll_merge_op *ops, int n_ops, int n_outer, const ll_lm_options *opt /* NULL: defaults */,
                       double *T_w7 /* [n_ops][7] out */, int *ran /* [n_ops], may be NULL */, ll_localize_fit *fit /* [n_ops], may be NULL */);
int  ll_cubemaps_align_timing(const ll_cubemaps *cms, double *ms /* build, search+fit, evaluate+solve, fit */, long long *counts /* stack points, map points, residual blocks */);

/* ---------------------------------------------------------------- measured information of a scan-to-map solve
 * ll_pose_info describes the residual blocks rebuilt at the FINAL pose of a localisation or an alignment -- the association pass the
 * fit record triggers, shared when both are asked for:
 *   H, g     what ll_map_normal_equations reports there: the Gauss-Newton Hessian J^T J, 6 x 6 row-major, and the gradient J^T r over the
 *            increment d = (w, dt) that ll_lm_solve_batch applies (q <- exp(w) (x) q with w the HALF-angle vector, t <- t + dt),
 *            HuberLoss(0.1) applied.  The same device functions sum them (ll_map_neq.h), in the solve's own order.
 *   rows     3 n_edge + n_plane
 *   sigma2   (sq_edge + sq_plane) / (rows - 6), the residual variance in m^2 (ll_localize_fit's sums, loss not applied); 0 when rows <= 6
 *   eig      the eigenvalues of H, ascending: cyclic Jacobi in f64 on one thread, 12 sweeps, the 15 rotations of a sweep in the order
 *            (0,1) (0,2) .. (4,5) -- the bits depend on H alone.  eig[0] small against eig[5] says that one direction of the pose is
 *            hardly constrained (a corridor, a straight road): the degeneracy test of Zhang, Kaess and Singh (ICRA 2016).
 *   flags    bit 0: H is not finite (eig is then all zero); bit 1: rows <= 6
 * WHAT IT IS: the information of the blocks at the final association.  It is right in SHAPE -- which directions the measurement fixes
 * and which it does not -- and optimistic in SCALE: wrong associations and errors of the map are not modelled, and neighbouring
 * residuals are far from independent.  ll_pg_edge_from_info's sigma is the caller's handle on the scale.
 *   ll_cubemaps_localize_slots_info   ll_cubemaps_localize_slots with info [S] (may be NULL: then it IS that call).  info != NULL adds one
 *            reduction launch (k_cms_info) behind the association pass at the final poses; the records come back in the copy that brings
 *            poses and fit, so the synchronisations stay three.  Poses, ran and fit are the same bits with or without info; a sequence
 *            that sat out or did not optimise gets an all-zero record; a view's record is the same bits alone and in any batch.
 *   ll_cubemaps_align_info            ll_cubemaps_align with info [n_ops] (may be NULL): k_al_eval<false> once more at the final T over the
 *            (op, chunk) workgroups, a one-wave sum per op in chunk order.  Still ONE synchronisation; n_outer = 0 gives the information
 *            at T0.  An op behind a shut gate gets an all-zero record.
 *   ll_drives_set_info / ll_drives_info   as ll_drives_fit: the last step's records [S], zeros for lanes that mapped, sat out or did not
 *            optimise.  Off after create; while off no launch is added and no bit changes, and ll_drives_info gives zeros.  Not part of a
 *            checkpoint.
 *   ll_pg_edge_from_info   the square-root information of the pose-graph edge (i -> j, Z = P_i^-1 X) that a record stands for; plain host
 *            arithmetic, no device, no context.  X_w7 is the solved pose H's increments refer to: the localised pose of the scan, or the
 *            aligned T (the quaternion is normalised here).  The edge error e = [2 sgn(w_e) vec(q_e) ; t_e] of E = X^-1 X' is, to first
 *            order in the increment d of X, e = M d with M = blkdiag(2 R(X)^T, R(X)^T); hence in the edge's own tangent
 *                Lambda = M^-T H M^-1 / sigma^2 + floor I,    M^-1 = blkdiag(R(X) / 2, R(X)),
 *            and S36 (row-major) is the upper-triangular Cholesky factor, S^T S = Lambda, for ll_pg_edge6.S.
 *            sigma > 0: the caller's residual standard deviation in metres; sigma <= 0: sqrt(info->sigma2), LL_ERR_STATE if that is 0.
 *            floor >= 0 is added to Lambda's diagonal and keeps a degenerate direction from making it singular.
 *            LL_ERR_STATE: flags bit 0, or Lambda is not positive definite.  LL_ERR_ARG: a NULL pointer, a non-finite argument or entry of
 *            X, a negative floor, a zero quaternion.                                                                                  */
typedef struct { double H[36]; double g[6]; double eig[6]; double sigma2; int rows; int flags; } ll_pose_info;
int  ll_cubemaps_localize_slots_info(ll_cubemaps *cms, const int *slots /* [S] */, const int *map_of /* [S], NULL: own map */,
                                     double *pose_w7 /* [S][7] */, int *ran /* [S], may be NULL */, ll_localize_fit *fit /* [S], may be NULL */,
                                     ll_pose_info *info /* [S], may be NULL */);
int  ll_cubemaps_align_info(ll_cubemaps *cms, const ll_merge_op *ops, int n_ops, int n_outer, const ll_lm_options *opt /* NULL: defaults */,
                            double *T_w7 /* [n_ops][7] out */, int *ran /* [n_ops], may be NULL */, ll_localize_fit *fit /* [n_ops], may be NULL */,
                            ll_pose_info *info /* [n_ops], may be NULL */);
int  ll_drives_set_info(ll_drives *d, int on);
int  ll_drives_info(ll_drives *d, ll_pose_info *info /* [S] */);
int  ll_pg_edge_from_info(const ll_pose_info *info, const double *X_w7, double sigma, double floor, double S36[36]);

/* ---------------------------------------------------------------- keyframes: the clouds every mapped frame contributed, kept on the device
 * A keyframe is what laserMapping adds to the map in its update (laserMapping.cpp:2103-2125): the frame's down-sized
 * laserCloudCornerStack and laserCloudSurfStack in the sensor frame -- what ll_cubemaps_download_cloud(q, 2 / 3) shows -- and the
 * pose_w7 the frame was mapped under.  ll_keyframes keeps them in two point pools in HBM (16 bytes per point, a frame's clouds back
 * to back in the order they were added) beside a host table; frame ids are 0 .. size - 1.  With them a map can be rebuilt under
 * corrected poses (ll_cubemaps_insert_keyframes below).  The store belongs to the context it was created on and works with the
 * ll_cubemaps / ll_drives of that context only (LL_ERR_ARG otherwise).
 *   ll_keyframes_create        max_frames in 1 .. 2^24, cap_corner / cap_surf (points) in 1 .. 2^30; LL_ERR_ARG (ll_last_error(ctx)) otherwise
 *   ll_keyframes_size          the number of frames (LL_ERR_ARG for NULL);  ll_keyframes_reset: size = 0, the pools empty
 *   ll_keyframes_info          frame id's table entry: host only, no launch, no synchronisation
 *   ll_keyframes_add_cubemaps  one keyframe per sequence with sel[q] = 1, ascending q, ids *first_id .. (first_id may be NULL; -1 when none
 *                              is selected): the sequence's current stack clouds, device to device in ONE copy launch for all sequences
 *                              and both types, no host synchronisation -- sizes and poses are host bookkeeping.  pose_w7 [S][7] (rows of
 *                              selected sequences are read), lane_tag / frame_tag [S] (NULL: the sequence index / -1) go into the table.
 *                              Between two frames of cms, or two steps of the ll_drives that owns it.
 *   ll_keyframes_add_points    one keyframe from host clouds (persistence, crafted tests): lane = -1, frame_index = -1; one synchronisation
 *   ll_keyframes_export        frames first .. first + count - 1 back to back, per frame the corner cloud and then the surf cloud:
 *                              offsets_out [2 count + 1] (cloud 2 f + w of the range begins at offsets_out[2 f + w]; the last entry is the
 *                              total) is host bookkeeping and always filled; points_out (host or device memory; NULL: sizes only, nothing
 *                              is launched) receives the points in one gather, one copy and ONE synchronisation whatever count is.
 *                              ll_keyframes_add_points of an exported frame stores the same bytes.
 * Errors, all decided before anything is enqueued; a refused call leaves size, table and pools as they were: LL_ERR_ARG for a NULL
 * pointer, a sel outside 0 / 1, a negative size, a range outside 0 .. size, a non-finite pose; LL_ERR_CAPACITY when max_frames or a
 * pool would overflow (last_error names which: "frames", "corner" or "surf"); LL_ERR_STATE for a selected sequence that has run no
 * frame since create / reset / import, or whose map is unusable.                                                                    */
typedef struct ll_keyframes ll_keyframes;
typedef struct { int max_frames; long long cap_corner, cap_surf; } ll_keyframes_params;
typedef struct { int lane, frame_index; int n[2]; long long offset[2]; double pose_w7[7]; } ll_keyframe_info;   /* n, offset: corner, surf; offset in points into the type's pool */
int  ll_keyframes_create(ll_ctx *ctx, const ll_keyframes_params *p, ll_keyframes **out);
void ll_keyframes_destroy(ll_keyframes *kf);
const char *ll_keyframes_last_error(const ll_keyframes *kf);
int  ll_keyframes_size(const ll_keyframes *kf);
int  ll_keyframes_reset(ll_keyframes *kf);
int  ll_keyframes_info(const ll_keyframes *kf, int id, ll_keyframe_info *info);
int  ll_keyframes_add_cubemaps(ll_keyframes *kf, ll_cubemaps *cms, const int *sel /* [S] */, const double *pose_w7 /* [S][7] */,
                               const int *lane_tag /* [S], may be NULL */, const int *frame_tag /* [S], may be NULL */, int *first_id);
int  ll_keyframes_add_points(ll_keyframes *kf, const ll_point *corner, int n_corner, const ll_point *surf, int n_surf, const double *pose_w7, int *id);
int  ll_keyframes_export(ll_keyframes *kf, int first, int count, ll_point *points_out, long long *offsets_out /* [2 count + 1] */);

/* ---------------------------------------------------------------- cube maps rebuilt and extended from keyframes
 * ll_cubemaps_insert_keyframes: op i places the listed frames of a store into map dst, each frame under its own pose.  The semantics
 * are ll_cubemaps_merge's with the source and the transform per frame.  Per cloud type (0 corner, 1 surf), independently:
 *   order      the points of the listed frames in list order, each frame's cloud in its own order.  Ids may repeat (the frame then
 *              contributes twice) and may come in any order;
 *   transform  pointAssociateToMap (laserMapping.cpp:125-134) in f64 with THAT FRAME's pose -- poses_w7[k] for frames[k], or the pose the
 *              store holds for the frame when poses_w7 is NULL -- used as given, never normalised; each coordinate rounded to float
 *              once, the fourth float carried over;
 *   binning    the cube arithmetic of :2108-2125 with dst's centre; a point outside the 21 x 21 x 11 array is dropped and counted;
 *   touched    every cube that receives a point becomes its old cloud followed by the new points in that order, passed ONCE
 *              through the library's VoxelGrid (:2151-2165) with the type's leaf.  A cube that receives nothing keeps its bytes.
 *   reset = 1  dst is first emptied as ll_cubemaps_reset does and given the centre cen (the array index of the world's origin cube:
 *              (10, 10, 5) puts the origin in the middle; a rebuild of a drive that has moved far passes the centre its map had,
 *              ll_cubemaps_layout): the valid list is empty and the four per-frame clouds are of size 0.
 *   reset = 0  the frames are added to what dst holds, cen is ignored: the map-extension case, and how a rebuild is split over calls.
 * FILTER ONCE, NOT FRAME BY FRAME: this is the merge's filter-once semantics -- all listed frames enter a cube before its one VoxelGrid
 * pass -- not the frame-by-frame VoxelGrid of incremental mapping, where every frame's update filters what the frames before left.  A
 * rebuild under the drive's own poses is therefore a map of the same points, not the same bytes as the incrementally built map.
 * added[i][w] / dropped[i][w] (either may be NULL): the points of op i, type w that entered a cube (before the filter) / fell outside.
 * Everything stays on the device: a workgroup of k_kf_assign takes one 1024-point tile of one (frame, type) cloud where it lies in
 * the store's pool; from the by-cube counting sort to the commit the call runs ll_cubemaps_merge's own stages.  Host synchronisations
 * per successful call that moves at least one point, whatever n_ops and the number of frames are: THREE (the per-cube counts, the
 * filtered sizes, the commit), plus the voxel filter's read-back as for a merge; all counted in ll_cubemaps_stats' syncs; frames does
 * not rise.  An op with no points succeeds (its reset is still made); a call whose ops hold no point at all launches nothing.
 * The handle from ll_drives_cubemaps(d) is accepted between any two ll_drives_step calls.
 * A failed call changes nothing, the reset included.  LL_ERR_ARG, before anything is enqueued: a NULL handle, store or ops, a store of
 * another context, n_ops < 1, n_frames < 0, frames NULL with n_frames > 0, a frame id outside the store, a non-finite pose (given or
 * stored), a dst outside 0 .. S-1, a dst listed by two ops, reset outside 0 / 1, a cen beyond +-2^24 with reset.  LL_ERR_STATE, also
 * before anything is enqueued: a dst that is unusable (an earlier update failed half-way).  LL_ERR_CAPACITY, decided for every op and
 * both types from the per-cube counts before any table changes -- with reset against the empty map --: last_error names the op and
 * the type.  LL_ERR_HIP: the workspace cannot be allocated (the object stays usable) or a runtime call failed.
 * ll_cubemaps_insert_timing: as ll_cubemaps_merge_timing, for the last insert.                                                   */
typedef struct { int dst; int n_frames; const int *frames; const double *poses_w7 /* [n_frames][7], NULL: the stored poses */;
                 int reset; int cen[3]; } ll_insert_op;
int  ll_cubemaps_insert_keyframes(ll_cubemaps *cms, const ll_keyframes *kf, const ll_insert_op *ops, int n_ops,
                                  long long *added /* [n_ops][2], may be NULL */, long long *dropped /* [n_ops][2], may be NULL */);
int  ll_cubemaps_insert_timing(const ll_cubemaps *cms, double *ms /* assign, sort+gather, filter, commit */, long long *counts /* points in, touched cubes, points out */);

/* ---------------------------------------------------------------- visibility: which stored points did other frames see through?
 * A map rebuilt from keyframes holds every point any frame contributed, a car that stood at a junction in one frame included.  A point
 * is not part of the static world if other frames looked straight through the place where it sits and measured something farther
 * away: the range-image visibility test of Removert (Kim & Kim, IROS 2020) and of Pomerleau et al. (ICRA 2014) -- not part of the
 * reference -- over what the store holds: per frame the down-sized corner and surf stacks in the sensor frame, and a pose.  The
 * evidence is therefore SPARSE; thresholds on real data are the caller's.  An ll_visibility belongs to ONE store (and its context).
 * THE IMAGE OF A FRAME (width columns over 360 degrees, height rows over el_min_deg .. el_max_deg).  For a point (x, y, z) in the
 * frame's sensor frame, in f32 with every product and sum rounded, left to right:
 *   r = sqrtf(x*x + y*y + z*z), used iff r >= min_range && r < max_range (a NaN is dropped);
 *   a = ll_atan2f(y, x), + 6.2831855f if negative;  col = min(width - 1, (int)(a * ka)), ka = (float)(width / (2 pi));
 *   h = sqrtf(x*x + y*y), e = ll_atan2f(z, h);  row = (int)floorf((e - el_min) * ke), el_min = (float)((double)el_min_deg * (pi / 180)),
 *   ke = (float)(height / (((double)el_max_deg - (double)el_min_deg) * (pi / 180))), pi / 180 and 2 pi as doubles; a row outside
 *   0 .. height - 1 gives no pixel;
 *   raw[row][col] = the minimum r over the points of BOTH of the frame's clouds in that pixel, +inf when empty -- an integer atomic
 *   minimum on the float's bits (ranges are positive: the unsigned order is the floats'), so it does not depend on the order of arrival;
 *   img[row][col] = the minimum of raw over the 3 x 3 pixels around it; columns wrap, rows outside the image are left out.  On sparse
 *   clouds the point's own pixel is not enough: ground at grazing angles is "seen through" by the pixel beside it.
 * THE VOTE (margin_abs, margin_rel, radius).  Subject point p of frame A with pose P_A; observer B: another frame of the same op --
 * "another" by position in the op's list -- with dx*dx + dy*dy + dz*dz <= (double)radius * (double)radius over the poses' translations
 * in f64, summed left to right, decided on the host.
 *   w = pointAssociateToMap(P_A, p) as ll_cubemaps_insert_keyframes has it: f64, each coordinate rounded to float once -- the
 *   numbers the insert bins;
 *   l = R(q_B)^-1 (w - t_B) in f64 from those floats: v = (double)w - t_B per coordinate, then the conjugate quaternion u = -(qx, qy, qz)
 *   with qw through the same operations in the same order: uv = u x v (uy*vz - uz*vy, ...), uv += uv,
 *   l = (float)((v + qw*uv) + u x uv) per coordinate; the pose is never normalised; each coordinate rounded to float once;
 *   l gives r, row, col as above; no evidence if l has no pixel, r is outside the range window, or d = img_B[row][col] is +inf;
 *   otherwise m = margin_abs + margin_rel * r (f32):  SEEN THROUGH by B if d > r + m;  HIT if d >= r - m && d <= r + m;  occluded
 *   otherwise, which is no evidence.
 * Per stored point two counters, through and hit, over all observers, each saturating at 255.  THE RULE: a point is removed iff
 * through >= min_through && hit <= max_hit; min_through in 1 .. 256 (256 never removes), max_hit in 0 .. 255 (255 ignores hits); the
 * default rule is {2, 255}.  A parked car that never moves is static by this test.
 *   ll_visibility_default_params  360 x 90 over -45 .. +45 degrees, ranges 1 .. 120, margins 0.5 + 0.02 r, radius 40, max_images 256
 *   ll_visibility_create     width in 8 .. 4096, height in 2 .. 1024, -89 <= el_min_deg < el_max_deg <= 89, max_images in 2 .. 2^16,
 *                            0 <= min_range < max_range, margins and radius finite and >= 0 (LL_ERR_ARG otherwise, ll_keyframes_last_error
 *                            of the store).  Two bytes per pool point ((cap_corner + cap_surf) * 2 bytes, zero) and max_images raw and
 *                            eroded images.  Destroy it before its store.
 *   ll_visibility_run        every op is one drive: its listed frames observe each other, frame k under poses_w7[k] (NULL: the stored
 *                            poses).  The counters of the listed frames are made anew (zero for an op with fewer than two frames or
 *                            no pair within radius); the counters of other frames keep their values; a frame that never took part has
 *                            zeros and is always kept.  pairs[i]: the ordered (subject, observer) frame pairs of op i.  The host builds
 *                            the cloud table and the observer lists (CSR over list positions) from the store's table; one upload, one
 *                            fill, THREE launches whatever n_ops is (k_vis_image, k_vis_erode, k_vis_vote), ONE synchronisation.  No
 *                            floating-point atomic: a frame's counters are the same bits alone, in any batch and in any order of ops.
 *   ll_visibility_counts     frame's counters, [n_corner + n_surf][2] bytes (through, hit), corner first; one synchronisation
 *   ll_visibility_images     raw / img [height][width] of the k-th listed frame, counted across ops, of the LAST run (tests, analysis);
 *                            one synchronisation
 *   ll_visibility_reset      all counters zero, the last run forgotten; the object follows the store again after ll_keyframes_reset
 *   ll_visibility_timing     the last run: ms = images, erode, vote (device events); counts = listed frames, their points, frame pairs
 *   ll_cubemaps_insert_keyframes_filtered   ll_cubemaps_insert_keyframes with the points the rule removes left out: a removed point
 *                            gets the key of a point outside the array in k_kf_assign, so every later stage is the plain insert's.
 *                            removed[i][w] counts them; dropped excludes them; added + dropped + removed = the listed points of the
 *                            type.  With nothing removed the maps are the plain insert's bytes.  Errors go to ll_cubemaps_last_error.
 * After ll_keyframes_reset the counters mean nothing: run, counts and the filtered insert return LL_ERR_STATE until
 * ll_visibility_reset.  Errors, all decided before anything is enqueued; a refused call leaves every counter as it was: LL_ERR_ARG for
 * a NULL handle or ops, n_ops < 1, n_frames < 0, frames NULL with frames to read, an id outside the store, an id listed twice in one
 * call (in one op or across ops), a non-finite pose, a rule outside its ranges, a store or visibility object of another store or
 * context; LL_ERR_CAPACITY for more listed frames than max_images; LL_ERR_HIP as elsewhere.                                         */
typedef struct ll_visibility ll_visibility;
typedef struct { int width, height; float el_min_deg, el_max_deg, min_range, max_range, margin_abs, margin_rel, radius; int max_images; } ll_visibility_params;
typedef struct { int n_frames; const int *frames; const double *poses_w7 /* [n_frames][7], NULL: the stored poses */; } ll_visibility_op;
typedef struct { int min_through, max_hit; } ll_visibility_rule;
void ll_visibility_default_params(ll_visibility_params *p);
int  ll_visibility_create(ll_keyframes *kf, const ll_visibility_params *p, ll_visibility **out);
void ll_visibility_destroy(ll_visibility *v);
const char *ll_visibility_last_error(const ll_visibility *v);
int  ll_visibility_run(ll_visibility *v, const ll_visibility_op *ops, int n_ops, long long *pairs /* [n_ops], may be NULL */);
int  ll_visibility_counts(ll_visibility *v, int frame, unsigned char *through_hit /* [n_corner + n_surf][2], corner first */);
int  ll_visibility_images(ll_visibility *v, int k, float *raw, float *img /* [height][width] each, either may be NULL */);
int  ll_visibility_reset(ll_visibility *v);
int  ll_visibility_timing(const ll_visibility *v, double *ms /* images, erode, vote */, long long *counts /* frames, points, pairs */);
int  ll_cubemaps_insert_keyframes_filtered(ll_cubemaps *cms, const ll_keyframes *kf, const ll_visibility *v, const ll_visibility_rule *rule,
                                           const ll_insert_op *ops, int n_ops, long long *added, long long *dropped,
                                           long long *removed /* [n_ops][2] each, may be NULL */);

/* ---------------------------------------------------------------- bev: from a place match to a guess, by correlative matching
 * A Scan Context match (ll_places) names the revisited scan and a heading good to a sector; the translation between the two sensor
 * positions is unknown and is metres on a real revisit, while ll_cubemaps_align and ll_cubemaps_localize_slots are local (a start
 * inside the 1 m association radius).  ll_bev closes that gap with correlative scan matching on bird's-eye occupancy grids (Olson,
 * ICRA 2009; the loop-closure matcher of Cartographer, Hess et al., ICRA 2016) -- not part of the reference -- over what an
 * ll_keyframes store holds.  An ll_bev belongs to ONE store (and its context).  Per op a QUERY (a list of stored frames) is matched
 * against a TARGET (a list of stored frames) over n_yaws x (2 sh)^2 rigid hypotheses (yaw_j, sx, sy); every score is a count, so
 * everything below is integers and exact.  All f32 arithmetic has every product and sum rounded, left to right.
 * A SIDE'S POINTS.  A side is a list of frame ids, the first is the ANCHOR; ids may repeat.  Frame k is under poses_w7[k], or under
 * its stored pose when the pointer is NULL.  Every point p of both stored clouds of every listed frame, the anchor included:
 *   w = pointAssociateToMap(P_k, p) as ll_cubemaps_insert_keyframes has it: f64, each coordinate rounded to float once;
 *   l = R(q_a)^-1 (w - t_a) with the anchor's pose, as the visibility vote spells it (above): f64 from those floats, each coordinate
 *   rounded to float once.  A point with a non-finite l coordinate is dropped before any conversion to integer.
 * CELLS AND LAYERS.  inv = (float)(1.0 / (double)cell), invz = (float)(1.0 / (double)z_layer);
 *   fx = floorf(x * inv), fy = floorf(y * inv), fl = floorf((z - z_min) * invz); every range test is made on the floats, then
 *   converted: a point HAS A LAYER iff 0 <= fl <= 7 (eight layers), and is INSIDE THE SQUARE iff -half <= fx, fy <= half - 1.
 * TARGET.  A byte per cell, [2 half][2 half]: bit fl of cell (fy + half, fx + half) is set for every target point that has a layer
 *   and lies inside the square (a 32-bit integer atomic OR: order-free).
 * QUERY.  Per point (x, y, layer) of l at the point's own position in a per-call list; the layer is -1 when the point is dropped or
 *   has no layer; no compaction.  n_query: the query points with a layer.
 * HYPOTHESES.  yaw_j = yaw0 + (double)j * yaw_step (host, f64), c_j = (float)cos(yaw_j), s_j = (float)sin(yaw_j) (libm).  For a query
 *   point with a layer: xr = c*x - s*y, yr = s*x + c*y, the cell (fx, fy) of (xr, yr); USED iff inside the square.
 * SCORE.  score[j][sy + sh][sx + sh], sx, sy in -sh .. sh - 1: the number of used query points whose bit `layer` is set in target
 *   cell (fx + sx, fy + sy); a cell outside the grid is empty.
 * PEAK.  The best hypothesis is the largest score; ties go to the lowest flat index (j, sy, sx).  second: the largest score among
 *   the hypotheses with |j - j*| > excl_yaw or |sx - sx*| > excl_shift or |sy - sy*| > excl_shift; -1 when there is none.
 *   second / score is the ambiguity handle -- a corridor or a straight road scores nearly as well one cell along -- and plays the
 *   role the eigenvalues play for the fine registration; thresholds on real data are the caller's.
 * RESULT.  yaw = yaw_{j*}; D_w7 = (0, 0, sin(yaw / 2), cos(yaw / 2), (double)sx * (double)cell, (double)sy * (double)cell, 0), host
 *   f64: p_target ~ D p_query, i.e. D measures P_target_anchor^-1 P_query_anchor in x, y and yaw.  Roll, pitch and z are NOT
 *   searched: the level-sensor assumption of Scan Context.  The guess for ll_cubemaps_align between two maps is
 *   T0 = P_c o D o P_q^-1 (ll_bev_guess); the start pose of a lane localising in the candidate's map is P_c o D.
 * WHY z_min = -1.  With the ground layer in, the sensor-centred ground rings of two scans coincide at ZERO shift whatever the true
 *   displacement is, and zero shift wins every time (the tests' yard scene: 6 896 hits at zero against 724 at the true displacement).  The
 *   default drops the ground of a sensor mounted about 1.8 m up; a caller with another mounting height changes z_min.
 *   ll_bev_default_params  cell 0.5, half 128, shift_half 16, z_min -1, z_layer 1, excl_yaw 1, excl_shift 2, max_ops 64, max_yaws 16,
 *                          max_points 2^21
 *   ll_bev_create     cell, z_layer finite and > 0, z_min finite, half in 1 .. 512, shift_half in 1 .. 16, excl_yaw, excl_shift >= 0,
 *                     max_ops in 1 .. 4096, max_yaws in 1 .. 64, max_points in 1 .. 2^30, and (2 half + 2 shift_half)^2 + 4096 bytes
 *                     within the 160 KiB of LDS (LL_ERR_ARG otherwise, ll_keyframes_last_error of the store).  Device memory is
 *                     taken by the first call that needs it and grown to the need.  Destroy it before its store.
 *   ll_bev_match      n_ops ops, one result each.  The host builds the tile table of the listed clouds, the poses, the op and yaw
 *                     tables; ONE upload, ONE fill (grids and counts), THREE launches whatever n_ops is -- k_bev_prepare (a workgroup
 *                     per 1024-point tile of one (op, side, frame, type) cloud where it lies in the store's pool), k_bev_score (a
 *                     workgroup per (op, yaw), a thread per shift, the op's grid resident in LDS inside a zero border of shift_half
 *                     cells, the query list staged 1024 entries at a time and walked by every thread) and k_bev_peak (a workgroup
 *                     per op) --, ONE synchronisation.  No floating-point atomic: an op's volume and result are the same bits
 *                     alone, at any position of any batch, and on every repetition.  An op whose query or target has no usable
 *                     point succeeds with score 0 and the best at flat index 0.
 *   ll_bev_volume     the scores [n_yaws][2 sh][2 sh] of op `op` of the LAST successful call (tests, analysis); one synchronisation
 *   ll_bev_grid       the target grid [2 half][2 half] of that op
 *   ll_bev_reset      the last call forgotten; the object follows the store again after ll_keyframes_reset
 *   ll_bev_timing     the last call: ms = prepare, score, peak (device events); counts = ops, listed points, hypotheses
 *   ll_bev_guess      T0 = P_c o D o P_q^-1 in the pose_w7 layout, host f64, no device, the poses used as given (unit quaternions
 *                     are the caller's): A o B = (q_A x q_B, R(q_A) t_B + t_A), the product spelled
 *                     (aw*bx + ax*bw + ay*bz - az*by, aw*by - ax*bz + ay*bw + az*bx, aw*bz + ax*by - ay*bx + az*bw,
 *                     aw*bw - ax*bx - ay*by - az*bz), R(q) v as pointAssociateToMap rotates; P^-1 = (q*, -(R(q*) t)); D o P_q^-1
 *                     first, then P_c o that.  LL_ERR_ARG for a NULL pointer.
 * Errors of ll_bev_match, all decided before anything is enqueued; a refused call launches nothing and leaves the last call's volume,
 * grids and timing readable: LL_ERR_ARG for a NULL handle, ops or out, n_ops outside 1 .. max_ops, a side with no frame or a NULL
 * list, an id outside the store, a non-finite pose (given or stored), a non-finite yaw0, yaw_step or yaw_j, n_yaws outside
 * 1 .. max_yaws; LL_ERR_CAPACITY for more listed points (both sides, all ops) than max_points; LL_ERR_STATE for match, volume and
 * grid after ll_keyframes_reset until ll_bev_reset or a new object; LL_ERR_ARG for a volume or grid of an op the last call did not
 * have; LL_ERR_HIP as elsewhere (the buffer cannot be grown: the last call is then forgotten).                                       */
typedef struct ll_bev ll_bev;
typedef struct { float cell; int half, shift_half; float z_min, z_layer; int excl_yaw, excl_shift, max_ops, max_yaws; long long max_points; } ll_bev_params;
typedef struct { int n_target; const int *target; const double *target_poses_w7 /* [n_target][7], NULL: the stored poses */;
                 int n_query;  const int *query;  const double *query_poses_w7 /* [n_query][7], NULL: the stored poses */;
                 double yaw0, yaw_step; int n_yaws; } ll_bev_op;
typedef struct { int score, second, iyaw, sx, sy, n_query; double yaw; double D_w7[7]; } ll_bev_result;
void ll_bev_default_params(ll_bev_params *p);
int  ll_bev_create(ll_keyframes *kf, const ll_bev_params *p, ll_bev **out);
void ll_bev_destroy(ll_bev *b);
const char *ll_bev_last_error(const ll_bev *b);
int  ll_bev_match(ll_bev *b, const ll_bev_op *ops, int n_ops, ll_bev_result *out /* [n_ops] */);
int  ll_bev_volume(ll_bev *b, int op, int *scores /* [n_yaws][2 sh][2 sh] */);
int  ll_bev_grid(ll_bev *b, int op, unsigned char *cells /* [2 half][2 half] */);
int  ll_bev_reset(ll_bev *b);
int  ll_bev_timing(const ll_bev *b, double *ms /* prepare, score, peak */, long long *counts /* ops, listed points, hypotheses */);
int  ll_bev_guess(const double *Pc_w7, const double *D_w7, const double *Pq_w7, double *T0_w7);

/* ---------------------------------------------------------------- entropy: how crisp is the cloud of these frames under these poses?
 * Ground truth free: a trajectory that lays the same wall down twice, 20 cm apart, makes thick point neighbourhoods, the corrected
 * one thin ones.  Mean map entropy (Droeschel, Stueckler & Behnke, ICRA 2014; Razlaw, Droeschel, Holz & Behnke, 2015) and mean plane
 * variance from the covariance of every point's fixed-radius neighbourhood -- not part of the reference -- over what an ll_keyframes
 * store holds.  The cube maps cannot show this (a double wall inside one voxel becomes one centroid).  An ll_entropy belongs to ONE
 * store (and its context).  WHAT IT IS NOT: it rewards any thinning, so compare trajectories over the same points only; thresholds on
 * real data are the caller's.
 * AN OP is (n_frames, frames, poses_w7) as an ll_visibility_op.  Its cloud is every corner and surf point of its listed frames, each
 * w = pointAssociateToMap(P_frame, p) as ll_cubemaps_insert_keyframes has it (f64, each coordinate rounded to float once).  Ops are
 * independent clouds: an id may occur once per op and in several ops (the same frames before and after a pose-graph solve, in one
 * call).  Every listed frame has a list position k counted across the ops, as ll_visibility_images counts it.
 * PER POINT q, in f32 with every operation rounded on its own:
 *   cell = radius * 1.03125f;  c = floorf(w / cell) per coordinate;  q is OUTSIDE if a coordinate of w is not finite or a c is not in
 *   -65536 .. 65535: nn = 0, h = pv = NaN, and it is nobody's neighbour;
 *   the neighbours of q are all points p of the same op that are not outside, q included, with d = p - q per coordinate and
 *   d2 = (dx*dx + dy*dy) + dz*dz <= radius * radius;
 *   over them, in f64 from those f32 d:  n,  S1 = sum d,  S2 = sum d d^T (products in f64: exact), in the order: cell rows dz, then
 *   dy ascending, a row's cells by x, a cell's points in list order;
 *   Sigma = S2 / n - (S1 / n)(S1 / n)^T entry by entry; its eigenvalues l0 <= l1 <= l2 by a cyclic Jacobi of 8 sweeps in f64;
 *   n >= min_neighbours: VALID, pv = (float)max(l0, 0), h = (float)(0.5 * (3 ln(2 pi e) + ln max(l0, f) + ln max(l1, f) + ln max(l2, f))),
 *   f = (double)lambda_floor;  otherwise SPARSE: nn set, h = pv = NaN.  nn is read as uint16 saturating at 65535.
 * PER OP an ll_entropy_rec: n_points = n_valid + n_sparse + n_outside;  n_pairs = the sum of the unsaturated nn of valid and sparse
 * points;  sum_h, sum_pv = f64 sums of the STORED f32 values of the valid points, in a fixed shape: per 1024-point tile of a (frame,
 * type) cloud thread t of 256 adds points t, t + 256, t + 512, t + 768 in that order from 0.0 and the 256 partials fold by halves
 * (t += t + 128, t += t + 64, ...); then the op's tiles in list order from 0.0;  mme = sum_h / n_valid, mpv = sum_pv / n_valid (0 when
 * n_valid is 0).  Nothing atomic, every sum in a fixed order: a point's values and an op's record are the same bits alone, in any
 * batch and at any op position.
 *   ll_entropy_default_params  radius 0.5, min_neighbours 6, lambda_floor 1e-6 (1 mm sigma), max_points 2^20
 *   ll_entropy_create     radius in (0, 8] (its f32 square at least 2^-100), min_neighbours >= 4 (fewer points have a singular
 *                         covariance), lambda_floor > 0 and finite, max_points in 1 .. 2^27 (LL_ERR_ARG otherwise,
 *                         ll_keyframes_last_error of the store).  The workspace, about 200 bytes per point, is sized from
 *                         max_points here and never grows.  Destroy it before its store.
 *   ll_entropy_run        at most 1024 ops; rec [n_ops].  The host builds the cloud table from the store's table; one upload and
 *                         keys, the stable sort by cell, heads + scan + cells, rows, moments, tile sums, op sums.  Host
 *                         synchronisations, whatever the numbers of ops and frames: TWO (the occupied-cell count that sizes the per-cell
 *                         launches; the records), plus the sort's read-back above 65536 points; ll_entropy_timing counts them.  A call
 *                         without a point launches nothing.
 *   ll_entropy_values     h, pv, nn [n_corner + n_surf] of the k-th listed frame of the LAST run, corner first; each may be NULL; one
 *                         synchronisation
 *   ll_entropy_reset      the last run forgotten; the object follows the store again after ll_keyframes_reset
 *   ll_entropy_timing     the last run: ms = keys, sort + cells, rows, moments, sums (device events); counts = listed frames, their
 *                         points, occupied cells, neighbour pairs, host synchronisations
 * After ll_keyframes_reset run and values return LL_ERR_STATE until ll_entropy_reset.  Errors, all decided before anything is enqueued;
 * a refused call leaves the last run's values readable and unchanged: LL_ERR_ARG for a NULL handle, ops or rec, n_ops < 1, n_frames < 0,
 * frames NULL with frames to read, an id outside the store, an id twice in one op, a non-finite pose (given or stored), a k the last
 * run did not have; LL_ERR_CAPACITY for more than 1024 ops or more listed points than max_points; LL_ERR_HIP as elsewhere.          */
typedef struct ll_entropy ll_entropy;
typedef struct { float radius; int min_neighbours; float lambda_floor; long long max_points; } ll_entropy_params;
typedef struct { int n_frames; const int *frames; const double *poses_w7 /* [n_frames][7], NULL: the stored poses */; } ll_entropy_op;
typedef struct { long long n_points, n_valid, n_sparse, n_outside, n_pairs; double sum_h, sum_pv, mme, mpv; } ll_entropy_rec;
void ll_entropy_default_params(ll_entropy_params *p);
int  ll_entropy_create(ll_keyframes *kf, const ll_entropy_params *p, ll_entropy **out);
void ll_entropy_destroy(ll_entropy *en);
const char *ll_entropy_last_error(const ll_entropy *en);
int  ll_entropy_run(ll_entropy *en, const ll_entropy_op *ops, int n_ops, ll_entropy_rec *rec /* [n_ops] */);
int  ll_entropy_values(ll_entropy *en, int k, float *h, float *pv, unsigned short *nn /* [n_corner + n_surf] each, each may be NULL */);
int  ll_entropy_reset(ll_entropy *en);
int  ll_entropy_timing(const ll_entropy *en, double *ms /* [5] keys, sort + cells, rows, moments, sums */,
                       long long *counts /* [5] frames, points, occupied cells, neighbour pairs, synchronisations */);

/* ---------------------------------------------------------------- drives: capture while driving, and take a correction
 * ll_drives_set_keyframes(d, kf, every): from the next step on, at the end of a step every lane that ran a frame -- mapping or
 * localising -- whose per-lane frame index (0 at START) is a multiple of every (>= 1) is captured into kf: its stack clouds and its
 * mapped_w7, tagged with lane and frame index, ids ascending with the lane.  One copy launch more per step, no host synchronisation
 * more.  kf = NULL: off, the default; off changes nothing by a bit.  Before anything of a step is enqueued the store must have room
 * for max_scan_corner / max_scan_surf points and one frame per lane the step would capture; otherwise the step fails with
 * LL_ERR_CAPACITY, has not run, and the lanes keep their state (the same commands can be given again).  The store is not part of a
 * lane checkpoint (the blob format is unchanged), and the setting is not either.  LL_ERR_ARG: every < 1, a store of another context.
 * ll_drives_correct(d, lanes, C_w7): left-multiplies the map-to-odom pose of every lane with lanes[q] = 1 by C_w7[q] on the device, in
 * f64: q' = q_C x q_m2o, t' = R(q_C) t_m2o + t_C (the products spelled as transformAssociateToMap spells them).  With
 * C = P'_last o P_last^-1 -- P_last the lane's last mapped pose, P'_last its corrected value -- the lane's next
 * transformAssociateToMap lands in the corrected map.  Allowed between any two steps for a lane that ran on the previous step or was
 * restored.  One tiny launch and one synchronisation (outside a step: not counted).  The identity (0, 0, 0, 1, 0, 0, 0) leaves every bit
 * of the lane's state unchanged.  LL_ERR_ARG, before anything is enqueued: a selector outside 0 / 1, a non-finite row of a selected
 * lane; LL_ERR_STATE: a selected lane with no drive.  C is not normalised.                                                        */
int  ll_drives_set_keyframes(ll_drives *d, ll_keyframes *kf /* NULL: off */, int every);
int  ll_drives_correct(ll_drives *d, const int *lanes /* [S] */, const double *C_w7 /* [S][7] */);

/* ---------------------------------------------------------------- place recognition: Scan Context descriptors, exhaustive matching
 * ll_places answers what comes before align, merge and set_localize: which stored scan is this scan a revisit of, and under which
 * heading.  It is the descriptor of Kim & Kim, "Scan Context" (IROS 2018) -- not part of the reference -- with an exact search of
 * every query against every stored place instead of the ring-key prefilter of the CPU implementations.
 * Descriptor: 20 rings x 60 sectors, desc[ring][sector], 1200 floats.  For a point (x, y, z), in f32 with every product and sum
 * rounded:  r = sqrtf(x*x + y*y), used iff r < max_radius (a NaN is dropped);  ring i = min(19, (int)(r / w)), w = max_radius / 20.0f
 * (the min only acts where the rounding of w lets r / w reach 20);  a = atan2f(y, x), +6.2831855f if negative;  sector
 * j = min(59, (int)(a * k)), k the float nearest to 60 / (2 pi);  desc[i][j] = the maximum over the bin's points of z + z_offset.  A bin
 * without points is 0.0f; one whose points all lie below -z_offset keeps its negative maximum.  z_offset is the sensor height.
 * Non-finite z, and non-finite uploaded descriptors, are outside the contract.  The source of ll_places_add_slots is a slot's resident
 * laserCloud (what ll_download_cloud returns); a slot whose scan was refused or is empty gives the all-zero descriptor, without a
 * read of its status by the host.  ll_places_add_points describes a host cloud through the same kernel.
 * Match-ready form, kept beside every descriptor and rebuilt by the same kernel after add and upload: norm_j = sqrtf of the sum over
 * rings 0 .. 19, in that order, of d*d in f32; column j divided by norm_j; a column with norm_j == 0 stays zero and counts as empty.
 * Distance of query Q and candidate C at shift s in 0 .. 59: over the columns j for which Q's column (j + s) mod 60 and C's column j
 * are both not empty (count of them), sim = the sum over j ascending of (unit column (j + s) mod 60 of Q) . (unit column j of C), a dot
 * product being an fmaf chain over rings 0 .. 19;  d(s) = 1.0f - sim / (float)count, 1.0f when count == 0.  The pair's result is
 * (min over s of d(s), the lowest s that reaches it).  If the query scan is the candidate scan turned by +phi about z,
 * p_q = Rz(phi) p_c, the minimum lies at s = phi / 6 degrees.  With P_q, P_c the two scans' poses in their maps, the transform from
 * the query's map to the candidate's is T0 = P_c Rz(-phi) P_q^-1; its translation is off by the distance between the two sensor
 * positions (metres), so it goes to ll_cubemaps_align as a small lattice of ops around T0 (n_outer = 0 scores a guess).
 * A pair's (distance, shift) has the same bits alone or inside any batch, whatever nq, nc and K are.
 *   ll_places_create     capacity places of 10 KB each in HBM; LL_ERR_ARG (ll_last_error(ctx)) for a capacity outside 1 .. 2^24 or
 *                        max_radius not positive and finite.  Destroy it before its context.
 *   ll_places_size       the number of places, ids 0 .. size - 1 (LL_ERR_ARG for NULL);  ll_places_reset: size = 0
 *   ll_places_add_slots  one place per entry of slots[count], ids consecutive from *first_id (may be NULL); one launch for all
 *   ll_places_add_points one place from n >= 0 host points
 *   ll_places_upload     count descriptors to ids first .. first + count - 1, first <= size: overwrites or extends
 *   ll_places_download   count descriptors from id first
 *   ll_places_distances  dist[nq][nc], shift[nq][nc] of queries q0 .. q0 + nq - 1 against candidates c0 .. c0 + nc - 1 of the same
 *                        database; LL_ERR_ARG when nq * nc exceeds 2^26
 *   ll_places_match      per query the K best candidates (1 <= K <= 8) by (distance, id) ascending: id[nq][K], dist[nq][K],
 *                        shift[nq][K]; ranks without a candidate hold id = -1, dist = +inf, shift = 0.  c_end NULL, or per query:
 *                        only candidate ids below c_end[q] are seen (a drive searching its own past without the last N frames).
 *                        The same nq * nc bound.
 *   ll_places_timing     ms[3]: device time of the last add / upload (describe + match-ready form; the call waits for it), of the
 *                        last search's Gram matrices and diagonals, and of the last match's selection; counts[2]: places of that
 *                        add, pairs of that search.  Either may be NULL.
 * add and upload enqueue on the context's stream and do not synchronise; download, distances and match synchronise ONCE per call,
 * whatever the sizes.  Errors are decided before anything is enqueued: LL_ERR_ARG for NULL handles or outputs, a slot outside the
 * context's batch, ranges outside 0 .. size, K outside 1 .. 8; LL_ERR_CAPACITY when an add or upload would exceed capacity (nothing
 * is added); LL_ERR_HIP when a workspace cannot be allocated.  ll_places_last_error has the text.
 * With ll_drives: a lane's laserCloud stays in the slot its raw scan was uploaded to until that row of the ring is reused two steps
 * later, so ll_places_add_slots takes the values ll_drives_slots returned BEFORE the step, after the step.                         */
typedef struct ll_places ll_places;
typedef struct { int capacity; float max_radius, z_offset; } ll_places_params;
void ll_places_default_params(ll_places_params *p, int capacity);      /* max_radius 80, z_offset 2 */
int  ll_places_create(ll_ctx *ctx, const ll_places_params *p, ll_places **out);
void ll_places_destroy(ll_places *db);
const char *ll_places_last_error(const ll_places *db);
int  ll_places_size(const ll_places *db);
int  ll_places_reset(ll_places *db);
int  ll_places_add_slots(ll_places *db, const int *slots, int count, int *first_id);
int  ll_places_add_points(ll_places *db, const ll_point *host, int n, int *id);
int  ll_places_upload(ll_places *db, int first, int count, const float *desc1200);
int  ll_places_download(ll_places *db, int first, int count, float *desc1200);
int  ll_places_distances(ll_places *db, int q0, int nq, int c0, int nc, float *dist, unsigned char *shift);
int  ll_places_match(ll_places *db, int q0, int nq, int c0, int nc, const int *c_end, int K, int *id, float *dist, unsigned char *shift);
int  ll_places_timing(ll_places *db, double *ms, long long *counts);

/* ---------------------------------------------------------------- pose graphs (ll_posegraph.hip; not in the reference)
 * Batched SE(3) pose-graph optimisation: what distributes a measured loop closure (ll_places_match + a localising lane) or a set of
 * session-to-session transforms (ll_cubemaps_align) over a trajectory.  n_graphs independent graphs per call, one workgroup each, the
 * whole Levenberg-Marquardt solve in one launch.
 *   A graph has N poses P_k = (q_k, t_k), world from body, in the pose_w7 layout (qx, qy, qz, qw, tx, ty, tz), and E edges.  Edge
 *   (i, j, Z_w7, sqrt_info, huber): Z measures P_i^-1 P_j; sqrt_info[6] is the DIAGONAL square-root information, rotation first, then
 *   translation; huber is the width a of ceres::HuberLoss, a <= 0 for none.  With E = Z^-1 P_i^-1 P_j = (q_e, t_e) the residual is
 *   r = sqrt_info o [2 sgn(w_e) vec(q_e) ; t_e] (sgn(0) = +1) and the cost 1/2 sum_e rho_a(|r_e|^2).  Increments are six per node
 *   (half-angle vector, then translation), applied as ll_lm_solve_batch applies them: q <- exp(d) (x) q, t <- t + dt.  Quaternions of
 *   poses and measurements are normalised on entry.  fixed[k] != 0 takes node k out of the problem.
 *   Layout of a call: node_off and edge_off have n_graphs + 1 ascending entries from 0 (ragged graphs back to back); poses_w7, fixed
 *   and edges are indexed by them; an edge's i, j are LOCAL to its graph.  fixed == NULL: node 0 of every graph is fixed.
 *   ll_pg_default_options   Ceres' trust-region defaults as ll_lm_default_options has them, 50 LM iterations, 1000 PCG iterations per
 *                           LM iteration, eta 0.1 (PCG stops at |r| <= eta |g|).  Needs no device.
 *   ll_posegraphs_create    device buffers for calls of at most max_graphs graphs with max_nodes_total nodes and max_edges_total
 *                           edges in all (about 850 B per node, 1.35 KB per edge: the upload holds either edge type).
 *   ll_posegraphs_evaluate  cost[n_graphs], the robustified cost of every graph at poses_w7, and grad6[nodes][6], its gradient with
 *                           respect to the increments (zeros at fixed nodes).  Solves nothing: the chi-square of a candidate loop edge
 *                           before it is accepted -- by the candidate's own information alone; ll_pg_edge_gate, below, also weighs
 *                           how uncertain the graph is about the two poses -- and the tests' window onto the Jacobians.
 *   ll_posegraphs_solve     optimises poses_w7 in place; rec (may be NULL) gets one record per graph: the cost at the start and at the
 *                           returned poses, the max-norm of Plus(x, -g) - x there, LM iterations, accepted steps, PCG iterations and
 *                           termination: 0 gradient_tolerance, 1 function_tolerance, 2 parameter_tolerance, 3 max_lm_iterations,
 *                           4 radius below min_radius, 5 a non-finite cost, gradient or step was met -- the poses are then the last
 *                           accepted ones (the input, if none was), never NaN.  Fixed nodes, nodes without an edge and every node of
 *                           a graph no step of which was accepted come back bit for bit.  opt == NULL: the defaults.
 *   ll_posegraphs_timing    ms[2]: device time of the last evaluate and of the last solve; counts[3]: graphs of the last call, LM and
 *                           PCG iterations of the last solve summed over its graphs.  Either may be NULL.
 * A graph's result does not depend on the batch: its poses and record have the same bits alone, in any batch, at any position.
 * evaluate and solve synchronise with the host ONCE per call, whatever the sizes.  Errors are decided on the host before anything is
 * enqueued and leave poses_w7 untouched; ll_posegraphs_last_error names the graph and the edge.  LL_ERR_ARG: a NULL pointer, offsets that
 * do not ascend from 0, an index outside its graph, i == j, a non-finite pose, measurement or weight, a zero quaternion, a graph without
 * a fixed node, options out of range.  LL_ERR_CAPACITY: the call exceeds a create-time total.  LL_ERR_HIP: an allocation failed.        */
typedef struct ll_posegraphs ll_posegraphs;
typedef struct { int i, j; double Z_w7[7]; double sqrt_info[6]; double huber; } ll_pg_edge;   /* i, j local to the graph */
typedef struct { int max_lm_iterations, max_pcg_iterations; double eta, initial_radius, max_radius, min_radius,
                 min_relative_decrease, min_lm_diagonal, max_lm_diagonal, function_tolerance, gradient_tolerance,
                 parameter_tolerance; } ll_pg_options;
typedef struct { double cost0, cost, grad_max; int lm_iterations, lm_successes, pcg_iterations, termination; } ll_pg_record;
void ll_pg_default_options(ll_pg_options *o);      /* Ceres' defaults where ll_lm_default_options has them; 50 LM, 1000 PCG, eta 0.1 */
int  ll_posegraphs_create(ll_ctx *ctx, int max_graphs, int max_nodes_total, int max_edges_total, ll_posegraphs **out);
void ll_posegraphs_destroy(ll_posegraphs *pg);
const char *ll_posegraphs_last_error(const ll_posegraphs *pg);
int  ll_posegraphs_evaluate(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, const double *poses_w7,
                            const unsigned char *fixed, const ll_pg_edge *edges, double *cost, double *grad6);
int  ll_posegraphs_solve(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, double *poses_w7,
                         const unsigned char *fixed, const ll_pg_edge *edges, const ll_pg_options *opt, ll_pg_record *rec);
int  ll_posegraphs_timing(ll_posegraphs *pg, double *ms2, long long *counts3);
/* The same two calls for edges with a FULL square-root information: r = S e with e = [2 sgn(w_e) vec(q_e) ; t_e] and S any finite 6 x 6
 * matrix, row-major (ll_pg_edge_from_info gives an upper-triangular one; diag(sqrt_info) is ll_pg_edge's residual).  Everything else --
 * the Huber scale, the slots, the node sums, PCG, the acceptance, the record, one workgroup per graph, one launch, no floating-point
 * atomic, the same bits alone and in any batch, ONE synchronisation, the errors and their order -- is the text above: the kernel is the
 * same template instantiated for this edge type, and ll_posegraphs_evaluate / _solve keep their own instantiation and bits.  A non-finite
 * entry of S is LL_ERR_ARG (last_error names the graph and the edge); an all-zero S is allowed: an edge that says nothing.              */
typedef struct { int i, j; double Z_w7[7]; double S[36]; double huber; } ll_pg_edge6;          /* i, j local to the graph */
int  ll_posegraphs_evaluate6(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, const double *poses_w7,
                             const unsigned char *fixed, const ll_pg_edge6 *edges, double *cost, double *grad6);
int  ll_posegraphs_solve6(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, double *poses_w7,
                          const unsigned char *fixed, const ll_pg_edge6 *edges, const ll_pg_options *opt, ll_pg_record *rec);
/* The preconditioner of the solves' conjugate gradients, a switch on the object (ll_pg_options and ll_pg_record keep their sizes).
 * LL_PG_PRECOND_BLOCK_JACOBI, the default, is the text above, unchanged by a bit.  LL_PG_PRECOND_CHAIN solves with M, the block-
 * tridiagonal part of A = H + D / radius in node order:
 *   diagonal block n     Hd[n] + diag(D[n]) / radius, what block-Jacobi inverts;
 *   coupling M[n][n+1]   the sum, in ascending edge order, over every edge whose endpoints are {n, n + 1} and both free: H_ij of an edge
 *                        with i == n, its transpose of one with i == n + 1 (duplicate edges sum);
 *   fixed nodes          an identity block, no coupling, a zero right-hand side: the chain breaks there;
 *   every other edge     (loop edges, edges that span more than one index) enters M through the diagonal blocks alone.
 * M is symmetric positive definite: the whole J^T J of the chain edges, plus the positive semi-definite diagonal parts of the others,
 * plus D / radius > 0.  A - M has rank at most 12 per other edge, so PCG needs at most 12 L + 1 iterations in exact arithmetic for L of
 * them, and one for a graph that is a chain; a graph without a chain edge gets block-Jacobi.  M^-1 is applied by block cyclic reduction
 * over the 6 x 6 blocks inside the graph's workgroup -- factorised once per LM iteration (M depends on the radius), applied once per PCG
 * iteration, ceil(log2 N) levels each way --: the same one launch, no grid barrier, no floating-point atomic, every sum of a fixed shape,
 * so a graph keeps the same bits alone, in any batch, at any position.  A Cholesky pivot that is not positive and finite (impossible in
 * exact arithmetic) makes the whole workgroup use block-Jacobi for that LM iteration, and is counted.
 *   ll_posegraphs_set_preconditioner  applies to _solve and _solve6 from the next call on; _evaluate and _evaluate6 solve nothing and do
 *                           not change.  The workspace (about 1.25 KB per node of max_nodes_total) is allocated when the chain is first
 *                           asked for.  LL_ERR_ARG: another kind; LL_ERR_HIP: the workspace cannot be allocated.  The old kind then stays.
 *   ll_posegraphs_preconditioner      the current kind, or a negative error code for a NULL handle.
 *   ll_posegraphs_precond_stats       counts2[0]: factorisations of M, counts2[1]: LM iterations that fell back to block-Jacobi, both
 *                           summed over the graphs of the last solve (zeros after a solve under block-Jacobi).
 *   ll_posegraphs_chain_solve         the solver alone, for direct tests and for callers with block-tridiagonal systems of their own:
 *                           n_systems independent symmetric positive definite systems, one workgroup each, through the device functions
 *                           the solves use.  node_off: n_systems + 1 ascending entries from 0, as above; diag36 [nodes][36]: the diagonal
 *                           blocks, row-major (the LOWER triangle is read); upper36 [nodes][36]: M[n][n+1], the last block of every
 *                           system ignored; rhs6 and out6 [nodes][6]; status [n_systems]: 0, or 1 where a pivot was not positive and
 *                           finite -- out6 of that system is then all zeros, the other systems are not touched by it.  A system's out6
 *                           has the same bits alone and in any batch.  ONE synchronisation.  Decided on the host before anything is
 *                           enqueued: LL_ERR_ARG for a NULL pointer, offsets that do not ascend from 0 or a non-finite entry (the ignored
 *                           blocks excepted); LL_ERR_CAPACITY for more than max_graphs systems or max_nodes_total nodes.  Allocates the
 *                           workspace if nothing has yet (LL_ERR_HIP).  Does not change the preconditioner of the solves.              */
#define LL_PG_PRECOND_BLOCK_JACOBI 0
#define LL_PG_PRECOND_CHAIN        1
int  ll_posegraphs_set_preconditioner(ll_posegraphs *pg, int kind);
int  ll_posegraphs_preconditioner(const ll_posegraphs *pg);
int  ll_posegraphs_precond_stats(ll_posegraphs *pg, long long counts2[2]);
int  ll_posegraphs_chain_solve(ll_posegraphs *pg, int n_systems, const int *node_off,
                               const double *diag36, const double *upper36,
                               const double *rhs6, double *out6, int *status);
/* The graph's own covariance: joint covariances of pose pairs (g2o's computeMarginals, Ceres' Covariance, GTSAM's Marginals), and the
 * Mahalanobis gate on a candidate loop edge that they make possible.
 *   H is the Gauss-Newton matrix the solves linearise at poses_w7: J^T J with the Huber scale, over the free nodes only, WITHOUT damping.
 *   Sigma = H^-1 is taken in the increments' own tangent: per node the half-angle vector, then the translation, applied on the left as
 *   the solves apply them (q <- exp(w) (x) q, t <- t + dt).  The rotation a half-angle vector w stands for is 2 w, so the covariance of
 *   the ROTATION VECTOR is 4 x the rotation block (and 2 x the rotation-translation blocks).
 *   ll_posegraphs_covariances   the call's layout is that of the solves (node_off, edge_off, poses_w7, fixed, edges; nothing is
 *                           modified).  q[n_queries]: (graph, a, b), a and b local to the graph, b < 0: node a alone.  joint144[q] is the
 *                           row-major 12 x 12 matrix [[S_aa, S_ab], [S_ba, S_bb]]; for b < 0 or b == a, S_aa sits in the top-left block
 *                           and the rest is zero.  A fixed node has zero rows and columns.  rec (may be NULL) gets one record per query:
 *                           status 0: every column converged; 1: some column stopped at max_pcg_iterations, the blocks are what the
 *                           conjugate gradients had; 2: breakdown (a p^T H p that is not positive and finite: H is singular or not
 *                           finite), the query's 144 numbers are zeros, never NaN.  pcg_iterations: summed over the query's columns (6 per
 *                           free node); residual: the largest final |r| among them.  opt == NULL: the defaults.
 *                           How: the (graph, node) sources of all queries are deduplicated on the host; k_pg_cov_prepare linearises every
 *                           queried graph once (and, under LL_PG_PRECOND_CHAIN, factorises the chain matrix at 1 / radius = 0 once); then
 *                           one workgroup per (source, k), k = 0 .. 5, solves H x = e_(source, k) by the solves' preconditioned conjugate
 *                           gradients under the object's preconditioner, until |r| <= tolerance (|b| = 1) -- the columns are independent
 *                           and fill the device where a lone solve uses one workgroup; a last kernel builds the 12 x 12: the diagonal
 *                           blocks symmetrised as (X + X^T) / 2, the cross block always from the columns of the smaller node index, so the
 *                           queries (a, b) and (b, a) are exact permutations of one another.  A graph whose chain matrix has a pivot that
 *                           is not positive and finite gets block-Jacobi for its columns.  Three launches, ONE synchronisation.  Every
 *                           index is relative to the graph and every sum has a fixed shape, without a floating-point atomic: a query's
 *                           144 numbers and record have the same bits alone, in any batch, at any position, beside any other queries.
 *                           The columns' workspace (1 728 B per source and node of its graph) is allocated at the first call and grown
 *                           when a call needs more; ll_posegraphs_create's sizes and the other calls' memory do not change.
 *                           Decided on the host before anything is enqueued, outputs untouched: the errors of the solves, and LL_ERR_ARG
 *                           for NULL queries or joint144, options out of range (max_pcg_iterations >= 1, tolerance >= 0 and finite), a
 *                           query's graph or node outside its range (a == b is allowed), or a queried node that no path of edges joins to
 *                           a fixed node -- H is singular there; last_error names the query and the node.  LL_ERR_HIP: the workspace cannot
 *                           be allocated.  n_queries == 0 is LL_OK and launches nothing.
 *   ll_posegraphs_covariances6  the same for ll_pg_edge6 graphs.
 *   ll_posegraphs_cov_timing    ms2: device time of the last call's prepare and of its columns; counts3: its queries, its deduplicated
 *                           free sources, the PCG iterations of all its columns.  Either may be NULL.
 *   ll_pg_edge_gate         plain host arithmetic, needs no device.  For a candidate edge a -> b with measurement Z_w7 and square-root
 *                           information S36 (row-major 6 x 6, r = S e; NULL: none) between poses whose joint covariance is joint144:
 *                           e is the edge's unweighted error, J = [J_a J_b] its unweighted Jacobians in the increments' tangent,
 *                           C = J Sigma J^T + (S^T S)^-1 (the second term absent for S36 == NULL), *chi2 = e^T C^-1 e, to be compared
 *                           with a chi-square quantile of 6 degrees of freedom (22.46 at 0.999); cov36 (may be NULL) gets C.  This is a
 *                           chi-square only for an edge that is NOT in the graph: Sigma of a graph that already holds the edge is not
 *                           independent of its error.  LL_ERR_ARG: a NULL pointer, a non-finite input, a zero quaternion, or a C or
 *                           S^T S that is not positive definite; the outputs are untouched then.                                     */
typedef struct { int graph, a, b; } ll_pg_cov_query;                  /* a, b local to the graph; b < 0: node a alone */
typedef struct { int max_pcg_iterations; double tolerance; } ll_pg_cov_options;          /* defaults 1000, 1e-10 */
typedef struct { int status, pcg_iterations; double residual; } ll_pg_cov_record;
void ll_pg_cov_default_options(ll_pg_cov_options *o);
int  ll_posegraphs_covariances(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, const double *poses_w7,
                               const unsigned char *fixed, const ll_pg_edge *edges, int n_queries, const ll_pg_cov_query *q,
                               const ll_pg_cov_options *opt, double *joint144, ll_pg_cov_record *rec);
int  ll_posegraphs_covariances6(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, const double *poses_w7,
                                const unsigned char *fixed, const ll_pg_edge6 *edges, int n_queries, const ll_pg_cov_query *q,
                                const ll_pg_cov_options *opt, double *joint144, ll_pg_cov_record *rec);
int  ll_posegraphs_cov_timing(ll_posegraphs *pg, double ms2[2], long long counts3[3]);
int  ll_pg_edge_gate(const double *Pa_w7, const double *Pb_w7, const double *Z_w7, const double *S36, const double joint144[144],
                     double *chi2, double cov36[36]);

/* ---------------------------------------------------------------- pcm: pairwise-consistent sets of loop-closure candidates
 * A revisit yields tens to thousands of candidate loop edges, some from look-alike places.  ll_pcm keeps a large mutually consistent set
 * of them BEFORE any enters a graph: pairwise consistency maximisation (Mangelson, Dominic, Eustice & Vasudevan, ICRA 2018) in the
 * threshold form of Kimera-RPGO's PcmSimple -- not part of the reference.  Two candidates are consistent if the cycle through both and
 * the trajectory between their endpoints closes.  Order of use: ll_pcm over all candidates, then ll_pg_edge_gate or a Huber width on the
 * survivors.  WHAT IT IS NOT: thresholds, not a Mahalanobis test (the measured information of ll_pose_info is not used); a greedy
 * clique, not the maximum one; and the nodes must be in trajectory order for L, below, to mean path length.  The default thresholds are
 * conventions (twice a 1 % drift), not measurements: thresholds on real data are the caller's.
 * A GRAPH of a call is N poses P in pose_w7, in trajectory order, and C <= 4096 candidates (i, j, Z_w7), Z measuring P_i^-1 P_j, i and j
 * local to the graph.  Only the poses are used, no edges.  The layout of a call is that of ll_posegraphs_*: node_off and cand_off have
 * n_graphs + 1 ascending entries from 0.
 * THE HOST, in plain f64 C before the upload: every quaternion (poses and Z) normalised, n = sqrt((x*x + y*y) + (z*z + w*w)), each
 * component / n;  the path length per graph, s[0] = 0, s[n+1] = s[n] + sqrt((dx*dx + dy*dy) + dz*dz) of the translations.
 * FROM THERE only + - * and comparisons in f64, every operation rounded on its own (ll_pcm_math.h is the text, shared by the kernels
 * and ll_pcm_host), so a decision has no sqrt and no division in it:
 *   a (x) b, quaternions (x, y, z, w):  x = aw*bx + ax*bw + ay*bz - az*by;  y = aw*by - ax*bz + ay*bw + az*bx;
 *                                       z = aw*bz + ax*by - ay*bx + az*bw;  w = aw*bw - ax*bx - ay*by - az*bz   (sums left to right)
 *   R(q) v:  r00 = 1 - 2*(y*y + z*z), r01 = 2*(x*y - z*w), r02 = 2*(x*z + y*w);  r10 = 2*(x*y + z*w), r11 = 1 - 2*(x*x + z*z),
 *            r12 = 2*(y*z - x*w);  r20 = 2*(x*z - y*w), r21 = 2*(y*z + x*w), r22 = 1 - 2*(x*x + y*y);  row k = (rk0*v0 + rk1*v1) + rk2*v2
 *   a o b = (q_a (x) q_b, R(q_a) t_b + t_a);   inv(a) = (q_a*, -(R(q_a*) t_a)),  q* = (-x, -y, -z, w)
 *   per candidate c:   B_c = Z_c o inv(P_jc);   Ai_c = (P_jc o inv(Z_c)) o inv(P_ic)
 *   per unordered pair, always evaluated as (c, d) with c < d:   E = (B_c o Ai_d) o P_ic  -- the cycle Z_c X(jc, jd) Z_d^-1 X(id, ic) in
 *   the body frame of i_c (the world-frame form Ai_d^-1 Ai_c would carry a lever arm of the world coordinates in its translation);
 *   rot2 = 4*((vx*vx + vy*vy) + vz*vz) of vec(q_E);  trans2 = (tx*tx + ty*ty) + tz*tz;  L = |s[ic] - s[id]| + |s[jc] - s[jd]|;
 *   ar = rot_tol + rot_rate*L;  at = trans_tol + trans_rate*L;
 *   CONSISTENT iff rot2 <= ar*ar && trans2 <= at*at and rot2, trans2, ar*ar, at*at are all finite (x - x == 0): huge finite inputs make
 *   an inconsistent pair, never a NaN decision.  The adjacency is symmetric by construction, its diagonal zero.
 * THE SELECTION, a deterministic greedy clique (Pattabiraman et al.'s heuristic as PCM uses it, every start tried): deg[c] = the
 * consistent partners of c;  the order is (deg descending, index ascending);  for every start v: M = {v}, U = N(v); while U is not
 * empty, u = the member of U earliest in the order, M += u, U = U & N(u);  the winner is the largest M, ties to the start earliest in the
 * order.  selected[c] = membership of the winner.  C == 0: nothing selected, start = -1; an isolated best gives a clique of 1 -- what
 * size means "confirmed" is the caller's.  An implementation may skip starts that cannot win; that changes work, never the result.
 * A BIT MATRIX of a graph is C rows of ceil(C / 64) 64-bit words, bit d % 64 of word d / 64 of row c standing for (c, d), in original
 * candidate order; the matrices of a call lie back to back.
 *   ll_pcm_default_params  rot_tol 0.05 rad, trans_tol 0.5 m, rot_rate 2e-4 rad/m, trans_rate 0.02
 *   ll_pcm_create      buffers for calls of at most max_graphs (1 .. 65535) graphs with max_nodes_total nodes and max_candidates_total
 *                      candidates in all (about 270 B per candidate); LL_ERR_ARG otherwise (ll_last_error(ctx)).  The bit matrices (16 B
 *                      per word of a call) are allocated at the first call and grown on demand.  Destroy it before its context.
 *   ll_pcm_run         selected [cands] (1: in the winner), degree [cands] (may be NULL), rec [n_graphs] (may be NULL); params NULL: the
 *                      defaults.  One upload, seven launches and a small clear whatever the number of graphs, ONE synchronisation.
 *   ll_pcm_select      the selection alone on caller-supplied bit matrices: for direct tests and for callers with a consistency test of
 *                      their own (as ll_posegraphs_chain_solve serves the chain solver)
 *   ll_pcm_adjacency   the bit matrix of one graph of the last run (or select) in original candidate order; one synchronisation;
 *                      LL_ERR_STATE before any call
 *   ll_pcm_timing      the last call: ms[5] = prepare, adjacency, order (degrees, ranks, the matrix in rank order), clique, pick (device
 *                      events; the first two are 0 after a select); counts[4] = graphs, candidates, pairs evaluated (C*C per graph: both
 *                      triangles), clique steps taken.  Either may be NULL.
 *   ll_pcm_host        one graph entirely on the host, needs no device: words_out (may be NULL), selected, degree (may be NULL), rec (may
 *                      be NULL) as ll_pcm_run gives them, bit for bit
 * A graph's matrix, selection, degrees and record have the same bits alone, in any batch and at any position: every index is relative
 * to the graph, the only atomics are integer, and none of them reaches a result.  Errors are decided on the host before anything is
 * enqueued and leave the outputs untouched; ll_pcm_last_error names the graph and the candidate.  LL_ERR_ARG: a NULL pointer, offsets
 * that do not ascend from 0, i or j outside the graph, i == j, a non-finite pose, Z or parameter, a negative parameter, a zero
 * quaternion; for select a matrix that is not symmetric, has a diagonal bit or a bit at or beyond C.  LL_ERR_CAPACITY: more than 4096
 * candidates in one graph, a call beyond a create-time total.  LL_ERR_HIP: the bit matrices could not be allocated.  n_graphs == 0 or
 * no candidate at all is LL_OK and launches nothing.                                                                              */
typedef struct ll_pcm ll_pcm;
typedef struct { double rot_tol, trans_tol, rot_rate, trans_rate; } ll_pcm_params;
typedef struct { int i, j; double Z_w7[7]; } ll_pcm_candidate;        /* i, j local to the graph */
typedef struct { int n_candidates, n_selected, start /* original index, -1: none */, max_degree; long long n_consistent_pairs; } ll_pcm_record;
void ll_pcm_default_params(ll_pcm_params *p);
int  ll_pcm_create(ll_ctx *ctx, int max_graphs, int max_nodes_total, int max_candidates_total, ll_pcm **out);
void ll_pcm_destroy(ll_pcm *pcm);
const char *ll_pcm_last_error(const ll_pcm *pcm);
int  ll_pcm_run(ll_pcm *pcm, int n_graphs, const int *node_off, const int *cand_off, const double *poses_w7,
                const ll_pcm_candidate *candidates, const ll_pcm_params *params, unsigned char *selected /* [cands] */,
                int *degree /* [cands], may be NULL */, ll_pcm_record *rec /* [n_graphs], may be NULL */);
int  ll_pcm_select(ll_pcm *pcm, int n_graphs, const int *cand_off, const unsigned long long *words, unsigned char *selected,
                   int *degree, ll_pcm_record *rec);
int  ll_pcm_adjacency(ll_pcm *pcm, int graph, unsigned long long *words_out);
int  ll_pcm_timing(const ll_pcm *pcm, double *ms /* [5] */, long long *counts /* [4] */);
int  ll_pcm_host(int n_nodes, const double *poses_w7, int n_candidates, const ll_pcm_candidate *candidates, const ll_pcm_params *params,
                 unsigned long long *words_out, unsigned char *selected, int *degree, ll_pcm_record *rec);

/* ---------------------------------------------------------------- whole hot path
 * One pass: extract + associate + vote + normal equations + one GN step for slots [first, first+count),
 * everything device-resident, no host synchronisation inside.  `vote_enable` as above.                   */
int ll_hot_path_batch(ll_ctx *ctx, int first, int count, const double *host_pose_guess, int vote_enable);
/* The same pass continuing a batch that an earlier call opened: the target of slot `first` is slot first - 1, not the carry
 * (a batch processed in pieces -- e.g. the halves of a double-buffered stream -- gives the results of one call over the whole). */
int ll_hot_path_chain(ll_ctx *ctx, int first, int count, int vote_enable);
/* Schedule of the association stage inside ll_hot_path_batch / _chain for calls (chunks) of at least 512 scans.  on = 0 (default): one
 * stream, kernel after kernel.  on = 1: the target grids of one quarter of the range are built while the quarter before it is searched,
 * on two HIP streams ordered by events.  Results are identical either way; on the MI355X boxes of round 6 the second schedule was never
 * faster (profiles/r06_experiments/two_stream_pieces.log), which is why it is not the default.  LIGHTLOAM_TWO_STREAM=1 in the environment
 * makes 1 the default of new contexts. */
int ll_set_two_stream(ll_ctx *ctx, int on);

/* ---------------------------------------------------------------- measurement
 * With profiling on, every kernel launched by the stage calls is bracketed by HIP events on the ctx stream.
 * ll_profile_read synchronises the stream and returns, per kernel, the summed duration and the launch count
 * since the last reset.  names[i] points to a static string.  n is in: capacity / out: kernels returned.    */
int ll_profile_enable(ll_ctx *ctx, int on);
int ll_profile_read(ll_ctx *ctx, int *n, const char **names, double *total_ms, int *launches, int reset);
/* 16 in-kernel phase counters (shader cycles); zero unless the library was built with -DLL_PHASE_TIMING (tools/phase_timing.py) */
int ll_debug_counters(ll_ctx *ctx, unsigned long long *out16, int reset);
/* one float4 streaming copy of `bytes` in + `bytes` out ("k_calib_copy"): the known-byte-count launch that calibrates
 * rocprofv3's FETCH_SIZE / WRITE_SIZE counters (tools/pmc_traffic.py) */
int ll_debug_calibration_copy(ll_ctx *ctx, unsigned long long bytes);
/* One stage's kernel(s) on their own over slots that hold what the stage reads: 0 organise, 1 pick, 2 voxel filter + lists, 3 grid tables,
 * 4 association, 5 vote, 6 normal equations (timing probes only; LL_ERR_ARG for another stage). */
int ll_debug_launch_stage(ll_ctx *ctx, int stage, int first, int count);
/* The DEVICE's evaluation of the arithmetic that must equal the host libm bit for bit (scanRegistration.cpp:139, :177 call
 * atan / atan2 / sqrt of glibc), over host arrays a, b, c (n floats each; unused ones may be NULL), results in out (n x 4 B):
 *   op 0  atanf(a)                    op 1  atan2f(a, b), general path     op 2  atan2f(a, b), k_classify's fast path
 *   op 3  (float)((double)a / M_PI)   op 4  a / sqrtf(b*b + c*c)  (:139's argument, z = a, x = b, y = c)
 *   op 5  ring id (int) of the point (x = b, y = c, z = a) by k_classify's threshold search with this context's parameters
 *   op 6  ring id (int) by evaluating the reference's formula chain directly on the device (:139-168)
 * Test surface (tests/test_gpu_a1_edges.py compares with glibc on the GPU box); not used by the pipeline. */
int ll_debug_exact_math(ll_ctx *ctx, int op, const float *a, const float *b, const float *c, int n, void *out);
/* The primitives under every map operation (the whole-cloud voxel filter, the sort by cube, merge, export, import), each on its own over
 * host arrays; every call allocates and frees its own workspace and synchronises once.  Test surface (tests/test_gpu_sort_scan.py,
 * tests/test_gpu_voxel.py); not used by the pipeline.
 *   ll_debug_sort_pairs      the stable sort of (u64 key, i32 value) pairs by key, in place.  seg_off == NULL: all n pairs in one sort (one
 *                            LDS workgroup up to 8192 pairs, eight LDS chunks and a merge up to 65536, device-wide radix passes above).
 *                            Else nseg + 1 host offsets: every segment [seg_off[s], seg_off[s + 1]) sorted on its own by one workgroup;
 *                            LL_ERR_ARG unless the offsets ascend from 0 to n, nseg is 1 .. 65535 and no segment exceeds 8192 pairs.
 *   ll_debug_exscan          the in-place exclusive prefix sum of n ints; LL_ERR_ARG for n < 0 or n > 4096 * 4096.
 *   ll_debug_voxel_segments  pcl::VoxelGrid of nseg clouds that lie back to back in `in` (offsets as above), as the cube-map stages call it:
 *                            the filtered clouds back to back in `out`, their sizes in seg_count[nseg], the total in *n_out.  max_seg_len is
 *                            handed on as those stages do: 1 .. 8192 (a bound on every segment, else LL_ERR_ARG) selects the sort per
 *                            segment when nseg > 1; 0, or more than 8192, the sort over all n.  LL_ERR_ARG for leaf <= 0 or bad offsets;
 *                            LL_ERR_CAPACITY, with *n_out set, when more than cap points result. */
int ll_debug_sort_pairs(ll_ctx *ctx, unsigned long long *keys, int *vals, int n, const int *seg_off, int nseg);
int ll_debug_exscan(ll_ctx *ctx, int *data, int n);
int ll_debug_voxel_segments(ll_ctx *ctx, const ll_point *in, int n, const int *seg_off, int nseg, float leaf, int max_seg_len,
                            ll_point *out, int cap, int *seg_count, int *n_out);

/* Algorithmic HBM bytes of the last ll_hot_path_batch / stage calls, summed over the slots they covered,
 * by SURVEY.md section 8d's formula (B_ext, B_assoc, B_vote, B_rj).                                      */
int ll_algorithmic_bytes(ll_ctx *ctx, int first, int count, double *b_ext, double *b_assoc, double *b_vote, double *b_rj);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTLOAM_HIP_H */
