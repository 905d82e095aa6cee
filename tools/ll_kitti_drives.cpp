// Many KITTI drives side by side: the directories of velodyne scans (*.bin, float32 x, y, z, reflectance) queued over `lanes`
// lanes of one lightloam::Drives (ll_drives), each through registration -> odometry -> mapping -- the many-drive twin of
//   ll_odometry_kitti <dir> <result_path> <scan_line> <first guess tx> 1 <max_ring_points>
// A lane starts the next directory of the queue when its drive ends.  Directory i's mapped trajectory goes to <result_dir>/<i>.txt
// in the reference's trajectory-file format (laserMapping.cpp:2284-2325), byte for byte what ll_odometry_kitti writes for it.
//
//   ll_kitti_drives [--maps] [--checkpoint FILE --checkpoint-at N] [--resume FILE] [--localize-in BLOB [--start-pose "qx qy qz qw x y z"] [--info]]
//                   [--distortion {0,1}] [--deskew {0,1,2}] [--map-vote N] <result_dir> <scan_line> <first-guess tx> <max_ring_points> <lanes> <dir>...
//
// --checkpoint FILE --checkpoint-at N: after step N (N >= 1 steps done) the lanes that ran on it are saved (ll_drives_save) to FILE
// together with the tool's own queue state -- per lane the drive it runs, its next frame and the first pose of its trajectory
// file --, and the run carries on.  --resume FILE (same lanes, same directories in the same order): the lanes are restored and the
// run continues with the frames after step N, appending to the pose files the first run began: a drive cut over several
// commands gives, byte for byte, the files of one uninterrupted command.  Both may be given: resume, then checkpoint again at a
// later step (N counts from the first run's start).
//
// --maps: when a drive ends, its final map (laserCloudMap, laserMapping.cpp:2190-2197: all cubes, corner then surf per cube) is
// also written, as <result_dir>/<i>_map.bin in the layout of the scans (float32 x, y, z, intensity: read_lidar_data reads it back).
// Lanes whose drives end on the same step are read in one export.  Without --maps the output is what it was.
//
// --localize-in BLOB: localise the drives in a saved map instead of mapping them.  BLOB is a file --checkpoint wrote (or a bare
// ll_drives_save blob); its R records are restored into lanes 0 .. R-1, which stay idle and keep their maps frozen; the drives run
// on the remaining lanes (lanes > R), each localising against record 0's map (ll_drives_set_localize): no map is written, any
// number of drives read the one map.  A drive begins at --start-pose in that map (seven numbers in one argument: quaternion x y z
// w, then x y z; identity when absent).  The trajectories are written as ever -- poses in the map's frame -- and beside each,
// <result_dir>/<i>_fit.txt with one line per frame: ran n_edge n_plane cost sq_edge sq_plane (ll_localize_fit), the answer to
// "am I still on the map?".  Not together with --checkpoint, --resume or --maps.
// --info (needs --localize-in): beside it <result_dir>/<i>_info.txt with one line per frame: eig[0] eig[5] sigma2 of the frame's
// ll_pose_info -- the smallest and the largest eigenvalue of the solve's Gauss-Newton Hessian and the residual variance in m^2 (zeros
// for a frame that did not optimise): "in which direction do I hardly know where I am?".
//
// --distortion 1: the reference's DISTORTION 1 path (ll_params.distortion) for a lidar whose scans are NOT motion-compensated (KITTI's
// are: leave it at 0).  --deskew 1 | 2 (needs --distortion 1, refused otherwise): TransformToEnd after every solved frame
// (ll_set_deskew) -- 1: the feature clouds the next frame and the mapper read, 2: also the full-resolution cloud.  A run resumed
// from a checkpoint takes the same two options again: the blob does not record the deskew mode.
//
// --map-vote N: the graph-based correspondence vote on the mapping stage's plane blocks (ll_drives_set_map_vote; laserMapping.cpp:836-1030,
// commented out in the reference) in every frame of a drive whose index is > N -- the reference's own gate is 20; the selected blocks
// replace the full list and keep stack order.  The surf capacity of the maps is then 116 000 points instead of 400 000: a twentieth of
// it must fit a workgroup's LDS.  Not recorded in a checkpoint: a resumed run takes the option again.  Localising lanes never vote.
//
// Build:  g++ -O2 -std=c++14 -I include tools/ll_kitti_drives.cpp -L light-loam_amd -llightloam_hip -o ll_kitti_drives
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dirent.h>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "lightloam_host.hpp"

static std::vector<std::string> bin_files(const std::string &dir)
{
    std::vector<std::string> files;
    if (DIR *d = opendir(dir.c_str())) {
        while (dirent *e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.size() > 4 && n.substr(n.size() - 4) == ".bin") files.push_back(dir + "/" + n);
        }
        closedir(d);
    }
    std::sort(files.begin(), files.end());
    return files;
}

/* the checkpoint file: the tool's queue state in front of the library's blob */
struct LaneState { int drive, frame, started; double H_init[12]; };
static const char CK_TAG[8] = {'L', 'L', 'K', 'D', '1', 0, 0, 0};

static void write_checkpoint(const std::string &path, long long steps, int next, const std::vector<LaneState> &lanes, const std::vector<unsigned char> &blob)
{
    std::FILE *f = std::fopen(path.c_str(), "wb");
    const int n = (int)lanes.size();
    const long long bytes = (long long)blob.size();
    const bool ok = f && std::fwrite(CK_TAG, 1, 8, f) == 8 && std::fwrite(&steps, sizeof(steps), 1, f) == 1 && std::fwrite(&next, sizeof(next), 1, f) == 1 &&
                    std::fwrite(&n, sizeof(n), 1, f) == 1 && std::fwrite(lanes.data(), sizeof(LaneState), lanes.size(), f) == lanes.size() &&
                    std::fwrite(&bytes, sizeof(bytes), 1, f) == 1 && std::fwrite(blob.data(), 1, blob.size(), f) == blob.size();
    if (f) std::fclose(f);
    if (!ok) throw lightloam::Error(LL_ERR_ARG, "cannot write " + path);
}

static void read_checkpoint(const std::string &path, long long &steps, int &next, std::vector<LaneState> &lanes, std::vector<unsigned char> &blob)
{
    std::FILE *f = std::fopen(path.c_str(), "rb");
    char tag[8];
    int n = 0;
    long long bytes = -1;
    bool ok = f && std::fread(tag, 1, 8, f) == 8 && std::memcmp(tag, CK_TAG, 8) == 0 && std::fread(&steps, sizeof(steps), 1, f) == 1 &&
              std::fread(&next, sizeof(next), 1, f) == 1 && std::fread(&n, sizeof(n), 1, f) == 1 && n >= 1 && n <= 4096;
    if (ok) { lanes.resize((size_t)n); ok = std::fread(lanes.data(), sizeof(LaneState), lanes.size(), f) == lanes.size() && std::fread(&bytes, sizeof(bytes), 1, f) == 1 && bytes >= 0 && bytes < (1LL << 40); }
    if (ok) { blob.resize((size_t)bytes); ok = std::fread(blob.data(), 1, blob.size(), f) == blob.size(); }
    if (f) std::fclose(f);
    if (!ok) throw lightloam::Error(LL_ERR_ARG, path + " is no ll_kitti_drives checkpoint");
}

int main(int argc, char **argv)
{
    bool maps = false, want_info = false;
    std::string ck_path, resume_path, loc_path, start_text;
    long long ck_at = -1;
    int distortion = 0, deskew = 0, map_vote = -1;
    while (argc > 1 && std::strncmp(argv[1], "--", 2) == 0) {
        const std::string opt = argv[1];
        if (opt == "--maps") { maps = true; --argc; ++argv; continue; }
        if (opt == "--info") { want_info = true; --argc; ++argv; continue; }
        if (argc < 3) { std::cerr << opt << " needs a value\n"; return 2; }
        if (opt == "--checkpoint") ck_path = argv[2];
        else if (opt == "--checkpoint-at") ck_at = std::atoll(argv[2]);
        else if (opt == "--resume") resume_path = argv[2];
        else if (opt == "--localize-in") loc_path = argv[2];
        else if (opt == "--start-pose") start_text = argv[2];
        else if (opt == "--distortion") distortion = std::atoi(argv[2]);
        else if (opt == "--deskew") deskew = std::atoi(argv[2]);
        else if (opt == "--map-vote") { map_vote = std::atoi(argv[2]); if (map_vote < 0) { std::cerr << "--map-vote takes a frame index >= 0\n"; return 2; } }
        else { std::cerr << "unknown option " << opt << "\n"; return 2; }
        argc -= 2; argv += 2;
    }
    if (ck_path.empty() != (ck_at < 1)) { std::cerr << "--checkpoint FILE and --checkpoint-at N (>= 1) go together\n"; return 2; }
    if (!loc_path.empty() && (maps || !ck_path.empty() || !resume_path.empty())) { std::cerr << "--localize-in does not go with --maps, --checkpoint or --resume\n"; return 2; }
    if (want_info && loc_path.empty()) { std::cerr << "--info needs --localize-in: only a localising lane measures its information\n"; return 2; }
    if (distortion < 0 || distortion > 1 || deskew < 0 || deskew > 2) { std::cerr << "--distortion takes 0 or 1, --deskew 0, 1 or 2\n"; return 2; }
    if (deskew != 0 && distortion == 0) { std::cerr << "--deskew " << deskew << " needs --distortion 1: without per-point interpolation ratios there is nothing to compensate\n"; return 2; }
    double start7[7] = {0, 0, 0, 1, 0, 0, 0};
    if (!start_text.empty()) {
        std::istringstream in(start_text);
        int got = 0;
        while (got < 7 && (in >> start7[got])) ++got;
        if (got != 7 || loc_path.empty()) { std::cerr << "--start-pose takes seven numbers in one argument and needs --localize-in\n"; return 2; }
    }
    if (argc < 7) { std::cerr << "usage: ll_kitti_drives [--maps] [--checkpoint FILE --checkpoint-at N] [--resume FILE] [--localize-in BLOB [--start-pose \"qx qy qz qw x y z\"] [--info]] [--distortion {0,1}] [--deskew {0,1,2}] [--map-vote N] <result_dir> <scan_line> <first-guess tx> <max_ring_points> <lanes> <dir>...\n"; return 2; }
    const std::string result_dir = argv[1];
    const int scan_line = std::atoi(argv[2]);
    const double tx0 = std::atof(argv[3]);
    const int max_ring_points = std::atoi(argv[4]), lanes = std::atoi(argv[5]);
    if (lanes < 1) { std::cerr << "lanes must be >= 1\n"; return 2; }
    std::vector<std::vector<std::string>> drives;
    for (int a = 6; a < argc; ++a) {
        drives.push_back(bin_files(argv[a]));
        if (drives.back().size() < 2) { std::cerr << "need at least two .bin scans in " << argv[a] << "\n"; return 2; }
    }
    try {
        using namespace lightloam;
        Context ctx(scan_line, 2 * lanes, 0, -1.0, -24.9f, 2.0f, distortion, max_ring_points, 3);   /* as ll_odometry_kitti: x, y, z resident */
        if (deskew != 0) ctx.set_deskew(deskew);                                           /* before any restore: it marks the slots it fills */
        Drives d(ctx, lanes, scan_line * 120 + 64, map_vote >= 0 ? 116000 : 400000, 1 << 22);   /* ll_odometry_kitti's mapping capacities; voting: a region must fit the LDS */
        if (map_vote >= 0) d.set_map_vote(map_vote);
        const double p0[7] = {0, 0, 0, 1, tx0, 0, 0};
        std::vector<double> pose0((size_t)7 * lanes);
        for (int q = 0; q < lanes; ++q) std::copy(p0, p0 + 7, &pose0[(size_t)7 * q]);
        std::vector<int> drive_of(lanes, -1), frame(lanes, 0);                             /* per lane: the drive it runs, its next frame */
        std::vector<std::unique_ptr<TrajectoryWriter>> out(drives.size());
        size_t next = 0;
        long long steps = 0;
        if (!resume_path.empty()) {                                                        /* the lanes as the saving run left them */
            std::vector<LaneState> st;
            std::vector<unsigned char> blob;
            int nxt = 0;
            read_checkpoint(resume_path, steps, nxt, st, blob);
            if ((int)st.size() != lanes || nxt < 0 || nxt > (int)drives.size()) throw Error(LL_ERR_ARG, resume_path + " was written for other lanes or directories");
            next = (size_t)nxt;
            std::vector<int> into;
            for (int q = 0; q < lanes; ++q) {
                if (st[q].drive < 0) continue;
                if (st[q].drive >= (int)drives.size() || st[q].frame < 1 || st[q].frame > (int)drives[st[q].drive].size() || !st[q].started)
                    throw Error(LL_ERR_ARG, resume_path + " was written for other lanes or directories");
                drive_of[q] = st[q].drive; frame[q] = st[q].frame; into.push_back(q);
                out[drive_of[q]].reset(new TrajectoryWriter(result_dir + "/" + std::to_string(drive_of[q]) + ".txt", st[q].H_init));
            }
            d.restore(blob, into);
        }
        int first_lane = 0;                                                                /* --localize-in: the lanes below hold the frozen maps */
        std::vector<std::unique_ptr<std::ofstream>> fit_out(drives.size()), info_out(drives.size());
        if (want_info) d.set_info(true);
        if (!loc_path.empty()) {
            std::vector<unsigned char> blob;
            try {                                                                          /* a file --checkpoint wrote ... */
                std::vector<LaneState> st; long long s0 = 0; int nxt = 0;
                read_checkpoint(loc_path, s0, nxt, st, blob);
            } catch (const Error &) {                                                      /* ... or a bare ll_drives_save blob */
                const std::vector<float> raw = read_lidar_data(loc_path);
                blob.assign((const unsigned char *)raw.data(), (const unsigned char *)raw.data() + raw.size() * sizeof(float));
            }
            ll_checkpoint_info info;
            std::memset(&info, 0, sizeof(info));
            if (ll_checkpoint_describe(blob.data(), (long long)blob.size(), &info) != LL_OK || info.n_records < 1) throw Error(LL_ERR_ARG, loc_path + " holds no checkpoint");
            if (info.n_records >= lanes) throw Error(LL_ERR_ARG, "--localize-in: " + std::to_string(info.n_records) + " records need more than " + std::to_string(info.n_records) + " lanes");
            first_lane = info.n_records;
            std::vector<int> into((size_t)first_lane);
            for (int r = 0; r < first_lane; ++r) into[(size_t)r] = r;
            d.restore(blob, into);
            std::vector<int> map_of(lanes, -1);
            std::vector<double> start((size_t)7 * lanes, 0.0);
            for (int q = 0; q < lanes; ++q) {
                std::copy(start7, start7 + 7, &start[(size_t)7 * q]);
                if (q >= first_lane) map_of[q] = 0;
            }
            d.set_localize(map_of, start.data());
        }
        for (;;) {
            std::vector<int> cmd(lanes, LL_DRIVE_IDLE);
            for (int q = first_lane; q < lanes; ++q) {
                if (drive_of[q] >= 0 && frame[q] < (int)drives[drive_of[q]].size()) { cmd[q] = LL_DRIVE_RUN; continue; }
                drive_of[q] = -1;
                if (next < drives.size()) {                                                 /* the lane takes the next drive of the queue */
                    drive_of[q] = (int)next++; frame[q] = 0; cmd[q] = LL_DRIVE_START;
                    const std::string path = result_dir + "/" + std::to_string(drive_of[q]) + ".txt";
                    std::remove(path.c_str());
                    out[drive_of[q]].reset(new TrajectoryWriter(path));
                    if (!loc_path.empty()) fit_out[drive_of[q]].reset(new std::ofstream(result_dir + "/" + std::to_string(drive_of[q]) + "_fit.txt", std::ios::trunc));
                    if (want_info) info_out[drive_of[q]].reset(new std::ofstream(result_dir + "/" + std::to_string(drive_of[q]) + "_info.txt", std::ios::trunc));
                }
            }
            if (std::all_of(cmd.begin(), cmd.end(), [](int c) { return c == LL_DRIVE_IDLE; })) break;
            const std::vector<int> slots = d.slots();
            for (int q = 0; q < lanes; ++q) {
                if (cmd[q] == LL_DRIVE_IDLE) continue;
                const std::vector<float> pts = read_lidar_data(drives[drive_of[q]][frame[q]]);
                ctx.check(ll_upload_scan(ctx.get(), slots[q], pts.data(), 4, (int)(pts.size() / 4)));
            }
            d.step(cmd, pose0.data());
            ++steps;
            const std::vector<ll_localize_fit> fit = loc_path.empty() ? std::vector<ll_localize_fit>() : d.fit();
            const std::vector<PoseInfo> info = want_info ? d.info() : std::vector<PoseInfo>();
            for (int q = 0; q < lanes; ++q) {
                if (cmd[q] == LL_DRIVE_IDLE) continue;
                out[drive_of[q]]->append(d.mapped_pose(q));
                if (!loc_path.empty()) {
                    char line[160];
                    std::snprintf(line, sizeof(line), "%d %d %d %.9e %.9e %.9e\n", d.ran[(size_t)q], fit[(size_t)q].n_edge, fit[(size_t)q].n_plane, fit[(size_t)q].cost,
                                  fit[(size_t)q].sq_edge, fit[(size_t)q].sq_plane);
                    *fit_out[drive_of[q]] << line << std::flush;
                    if (want_info) {
                        std::snprintf(line, sizeof(line), "%.9e %.9e %.9e\n", info[(size_t)q].eig[0], info[(size_t)q].eig[5], info[(size_t)q].sigma2);
                        *info_out[drive_of[q]] << line << std::flush;
                    }
                }
                ++frame[q];
            }
            if (steps == ck_at) {                                                           /* the lanes that ran on this step, and the queue */
                std::vector<LaneState> st((size_t)lanes);
                std::vector<int> sel(lanes, 0);
                for (int q = 0; q < lanes; ++q) {
                    std::memset(&st[q], 0, sizeof(LaneState));
                    st[q].drive = -1;
                    if (cmd[q] == LL_DRIVE_IDLE) continue;
                    sel[q] = 1; st[q].drive = drive_of[q]; st[q].frame = frame[q]; st[q].started = out[drive_of[q]]->started() ? 1 : 0;
                    std::copy(out[drive_of[q]]->init(), out[drive_of[q]]->init() + 12, st[q].H_init);
                }
                write_checkpoint(ck_path, steps, (int)next, st, d.save(sel));
            }
            if (maps) {                                                                     /* the drives that just ended: their maps, before a START clears them */
                std::vector<int> which(lanes, LL_MAP_NONE);
                bool any = false;
                for (int q = 0; q < lanes; ++q)
                    if (cmd[q] != LL_DRIVE_IDLE && frame[q] == (int)drives[drive_of[q]].size()) { which[q] = LL_MAP_ALL; any = true; }
                if (any) {
                    std::vector<PointXYZI> pts;
                    std::vector<long long> off;
                    d.export_maps(which, pts, off);
                    for (int q = 0; q < lanes; ++q) {
                        if (which[q] != LL_MAP_ALL) continue;
                        const std::string path = result_dir + "/" + std::to_string(drive_of[q]) + "_map.bin";
                        std::FILE *f = std::fopen(path.c_str(), "wb");
                        const size_t n = (size_t)(off[(size_t)q + 1] - off[(size_t)q]);
                        if (!f || std::fwrite(pts.data() + off[(size_t)q], sizeof(PointXYZI), n, f) != n) { if (f) std::fclose(f); throw Error(LL_ERR_ARG, "cannot write " + path); }
                        std::fclose(f);
                    }
                }
            }
        }
        long long syncs = 0, frames = 0;
        d.stats(syncs, frames);
        std::cout << "wrote " << drives.size() << " mapped trajectories to " << result_dir << " in " << steps << " steps over " << lanes
                  << " lanes (" << syncs << " host synchronisations)\n";
    } catch (const lightloam::Error &e) {
        std::cerr << "lightloam error " << e.code << ": " << e.what() << "\n";
        return 1;
    }
    return 0;
}
