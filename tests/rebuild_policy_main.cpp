// rebuild_policy_main.cpp — the drift rebuild policy (prosper_amd/csrc/pt_rebuild_policy.hpp: what stage_transforms and
// prosper_pt_animate act on) over all of its inputs, on a CPU.  tests/test_rebuild_policy.py holds the table.
//
//   rebuild_policy <threshold> <below> <above>
//
// One line per input, 2^5 booleans x the ratios below, equal to and above the threshold:
//   moved alwaysRebuild driftSite gpuBuilder buildRunning ratio(0 below, 1 equal, 2 above) decision(None, Synchronous, Background)
#include <cstdio>
#include <cstdlib>

#include "pt_rebuild_policy.hpp"

using namespace ppt;

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const float threshold = std::strtof(argv[1], nullptr);
    const float ratios[3] = {std::strtof(argv[2], nullptr), threshold, std::strtof(argv[3], nullptr)};
    if (!(ratios[0] < threshold && threshold < ratios[2])) return 2;
    for (unsigned bits = 0; bits < 32u; ++bits)
        for (int r = 0; r < 3; ++r)
        {
            const bool moved = bits & 1u, always = bits & 2u, drift = bits & 4u, gpu = bits & 8u, running = bits & 16u;
            const RebuildDecision d = rebuild_policy(moved, ratios[r], threshold, always, drift, gpu, running);
            const char *name = d == RebuildDecision::None ? "None" : d == RebuildDecision::Synchronous ? "Synchronous" : "Background";
            std::printf("%d %d %d %d %d %d %s\n", moved, always, drift, gpu, running, r, name);
        }
    return 0;
}
