// launch_plan_shim.cpp — tests/test_launch_plan.py's way into rayzath_amd/csrc/hiprz_plan.cpp: a program of its own (compiled with the
// unit under sanitizers, run as a child process) that reads an array of hiprz::PlanInputs records from a file and writes the
// hiprz::LaunchPlan of each to another.
//   launch_plan_shim IN OUT COUNTED    (COUNTED: 0 | 1)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hiprz_plan.hpp"

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 3;
    const bool counted = std::atoi(argv[3]) != 0;
    std::vector<hiprz::PlanInputs> records(4096);
    std::vector<hiprz::LaunchPlan> plans(records.size());
    size_t total = 0;
    for (size_t n; (n = std::fread(records.data(), sizeof(hiprz::PlanInputs), records.size(), in)) != 0; total += n) {
        for (size_t i = 0; i < n; ++i) plans[i] = hiprz::plan_launches(records[i], counted);
        if (std::fwrite(plans.data(), sizeof(hiprz::LaunchPlan), n, out) != n) return 4;
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 4;
    std::printf("%zu %zu %zu\n", sizeof(hiprz::PlanInputs), sizeof(hiprz::LaunchPlan), total);
    return 0;
}
