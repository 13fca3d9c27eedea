// Stand-alone driver of the sealed-pointing registry's selftest (toast_amd/csrc/pointing_cache.cpp) for sanitizer builds:
// the registry is host code without a HIP call, so it links without the rest of the library and runs without a device.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itoast_amd/csrc
//       toast_amd/csrc/pointing_cache.cpp tools/pointing_cache_selftest.cpp -o pointing_cache_selftest   (one line)
//   ./pointing_cache_selftest [n_seeds] [n_ops]
//
// Exit status 0 = every named scenario (1-10) and every random sequence was sound.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "pointing_cache.hpp"

int main(int argc, char ** argv) {
    const int n_seeds = argc > 1 ? std::atoi(argv[1]) : 40;
    const int n_ops = argc > 2 ? std::atoi(argv[2]) : 6000;
    int bad = 0;
    for (int which = 1; which <= 10; ++which) {
        const std::string e = toast_hip::pointing_cache::selftest(0, 0, which);
        if (!e.empty()) {
            std::printf("scenario %d: %s\n", which, e.c_str());
            ++bad;
        }
    }
    for (int seed = 1; seed <= n_seeds; ++seed) {
        const std::string e = toast_hip::pointing_cache::selftest((uint64_t)seed, n_ops, 0);
        if (!e.empty()) {
            std::printf("seed %d: %s\n", seed, e.c_str());
            ++bad;
        }
    }
    std::printf("%d scenarios + %d sequences of %d steps: %s\n", 10, n_seeds, n_ops, bad == 0 ? "sound" : "BROKEN");
    return bad == 0 ? 0 : 1;
}
