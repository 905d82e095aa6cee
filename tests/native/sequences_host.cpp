// lightloam::odometry_sequences from C++ (include/lightloam_host.hpp):
//   sequences_host <dir> <scan_line> <n_seq> <n_frames>
// <dir>/s<q>_f<k>.bin: KITTI-format frame k of sequence q; <dir>/pose0.bin: n_seq x 7 doubles, the warm start of frame 1.
// Frames go into a ring of n_frames rows (row k = frame k), rows 1 .. n_frames - 1 run; prints one line per (row, sequence):
// the 7 pose values with 17 significant digits.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "lightloam_host.hpp"

template <typename T>
static std::vector<T> read_all(const std::string &path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) { std::cerr << "cannot open " << path << "\n"; std::exit(2); }
    const std::streamsize bytes = f.tellg();
    f.seekg(0);
    std::vector<T> v((size_t)bytes / sizeof(T));
    f.read((char *)v.data(), bytes);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 5) { std::cerr << "usage: sequences_host dir scan_line n_seq n_frames\n"; return 2; }
    const std::string dir = argv[1];
    const int rings = std::atoi(argv[2]), S = std::atoi(argv[3]), N = std::atoi(argv[4]);
    try {
        std::vector<std::vector<float> > scans;
        for (int k = 0; k < N; ++k)
            for (int q = 0; q < S; ++q) scans.push_back(read_all<float>(dir + "/s" + std::to_string(q) + "_f" + std::to_string(k) + ".bin"));
        const std::vector<double> pose0 = read_all<double>(dir + "/pose0.bin");
        lightloam::Context ctx(rings, S * N);
        ll_seq_layout L;
        L.base = 0; L.n_seq = S; L.ring_rows = N;
        for (int k = 0; k < N; ++k)
            for (int q = 0; q < S; ++q) {
                const std::vector<float> &p = scans[(size_t)k * S + q];
                ctx.check(ll_upload_scan(ctx.get(), L.base + k * S + q, p.data(), 4, (int)(p.size() / 4)));
            }
        ctx.check(ll_extract_batch(ctx.get(), 0, S * N));
        const std::vector<double> rel = lightloam::odometry_sequences(ctx, L, 1, N - 1, nullptr, nullptr, pose0.data());
        for (size_t i = 0; i < rel.size() / 7; ++i) {
            for (int k = 0; k < 7; ++k) std::printf(k == 6 ? "%.17g\n" : "%.17g ", rel[i * 7 + k]);
        }
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    return 0;
}
