// codec_eval_report.hpp's image-heuristics CSV writer on fixed rows; tests/test_image_heuristics_cpu.py compares its
// output with reports.heuristics_csv on the same rows.
#include <cmath>
#include <cstdio>

#include "codec_eval_report.hpp"

int main()
{
    ce_image_heuristics a{}, b{};
    a.width = 3, a.height = 4, a.pixels = 12;
    a.mean_luminance = 0.125f, a.luminance_variance = 0.375f, a.luminance_std = 2.5f, a.edge_strength_mean = 1.005f;
    a.edge_strength_max = 255.0f, a.edge_density = 0.03125f, a.flat_block_pct = 100.0f, a.saturation_mean = 0.41576192f;
    a.freq_ratio = std::nanf(""), a.diagonal_complexity = 1234.5678f;
    b.width = 768, b.height = 512, b.pixels = 393216;
    b.high_freq_energy = 0.0625f, b.low_freq_energy = 0.9375f;
    std::fputs(codec_eval::report::heuristics_csv({{"a.png", a}, {"b c.jpg", b}}).c_str(), stdout);
    return 0;
}
