// calculate_ssimulacra2_with_maps of the C++ host mirror (codec-eval_amd/host/codec_eval.hpp) on one pair of RGB8 files:
// prints the score, the 108 features (floats as C99 hex) and "w h" per scale, and writes every scale's nine maps to
// <out_dir>/scale<s>.f32.  Driven by tests/test_gpu_ssimulacra2_maps.py, which compares all of it with the Python binding.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "codec_eval.hpp"

using namespace codec_eval;
using namespace codec_eval::metrics;

static Bytes read_file(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    return Bytes(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv)
{
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s ref.rgb test.rgb width height out_dir\n", argv[0]);
        return 2;
    }
    const Bytes ref = read_file(argv[1]), test = read_file(argv[2]);
    const size_t w = std::stoul(argv[3]), h = std::stoul(argv[4]);
    try {
        HipBackend be(0);
        const Ssim2WithMaps r = calculate_ssimulacra2_with_maps(be, ref, test, w, h);
        std::printf("%a\n", r.score);
        for (double f : r.features) std::printf("%a\n", f);
        for (size_t s = 0; s < r.scales.size(); s++) {
            const Ssim2Maps &m = r.scales[s];
            if (m.maps.size() != 9 * m.width * m.height) return 3;
            std::printf("%zu %zu\n", m.width, m.height);
            std::ofstream o(std::string(argv[5]) + "/scale" + std::to_string(s) + ".f32", std::ios::binary);
            o.write(reinterpret_cast<const char *>(m.maps.data()), (std::streamsize)(m.maps.size() * sizeof(float)));
        }
        bool threw = false;  // a length error comes back as the mirror's exception
        try {
            calculate_ssimulacra2_with_maps(be, ref, Bytes(test.begin(), test.end() - 3), w, h);
        } catch (const std::exception &) {
            threw = true;
        }
        if (!threw) return 4;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
