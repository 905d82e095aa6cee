/* lightloam::LaserMappingSequences::align_maps on two imported maps (tests/test_gpu_map_align.py writes them and compares the
 * result bit for bit with CubeMaps.align): argv[1] holds map0.bin / map1.bin (float32 x, y, z, intensity in LL_MAP_ALL order),
 * layout0.bin / layout1.bin (int32: centre [3], counts [2][4851]) and guess.bin (7 doubles); result.bin receives T [7], ran,
 * n_edge, n_plane, cost, sq_edge, sq_plane as doubles. */
#include "lightloam_host.hpp"
#include <cstdio>
#include <string>

template <typename T>
static std::vector<T> read_all(const std::string &path)
{
    std::vector<T> v;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path.c_str()); std::exit(2); }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(T));
    if (bytes > 0 && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) { std::fprintf(stderr, "short read of %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    try {
        lightloam::Context ctx(16, 1);
        lightloam::LaserMappingSequences maps(ctx, 2, 0.4f, 0.8f, 64, 64, 1 << 15);
        std::vector<lightloam::PointXYZI> points;
        std::vector<long long> offset(1, 0);
        lightloam::MapLayout layout[2];
        for (int q = 0; q < 2; ++q) {
            const std::vector<lightloam::PointXYZI> p = read_all<lightloam::PointXYZI>(dir + "/map" + std::to_string(q) + ".bin");
            const std::vector<int> l = read_all<int>(dir + "/layout" + std::to_string(q) + ".bin");
            if (l.size() != 3 + (size_t)lightloam::MapLayout::N_COUNTS) return 2;
            points.insert(points.end(), p.begin(), p.end());
            offset.push_back((long long)points.size());
            for (int k = 0; k < 3; ++k) layout[q].cen[k] = l[k];
            layout[q].counts.assign(l.begin() + 3, l.end());
            layout[q].valid.clear();
        }
        maps.import_maps(points, offset, {&layout[0], &layout[1]});
        const std::vector<double> guess = read_all<double>(dir + "/guess.bin");
        std::vector<ll_merge_op> ops(1);
        ops[0].dst = 0; ops[0].src = 1;
        for (int k = 0; k < 7; ++k) ops[0].T_w7[k] = guess[k];
        std::vector<double> T;
        std::vector<int> ran;
        std::vector<ll_localize_fit> fit;
        maps.align_maps(ops, 2, &T, &ran, &fit);
        std::vector<double> out(T.begin(), T.end());
        out.push_back((double)ran[0]);
        out.push_back((double)fit[0].n_edge); out.push_back((double)fit[0].n_plane);
        out.push_back(fit[0].cost); out.push_back(fit[0].sq_edge); out.push_back(fit[0].sq_plane);
        FILE *f = std::fopen((dir + "/result.bin").c_str(), "wb");
        if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 3;
        std::fclose(f);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
