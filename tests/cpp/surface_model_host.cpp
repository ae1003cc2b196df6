// surface_model_host.cpp -- the surface fuzzer's generator and model (tests/cpp/surface_model.h) without a device, a plain
// executable built with the address and undefined-behaviour sanitizers.
//
//   surface_model_host --plan-only [--seed S] [--cases N] [--case K] [--class tiny|small|mid]
//       draws the cases fuzz_surface would run, applies them to the model and prints the coverage table and the share of
//       finite float elements among everything a run compares: both are settled here, without a GPU
//   surface_model_host --dump FILE [...]
//       also writes every case's statements and the model's final pool as JSON (values as bit patterns), for a replay elsewhere
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "surface_model.h"

using namespace sfm;

template <typename T> void run_case(std::uint64_t seed, std::uint64_t k, Coverage &cov, std::ostream *dump, bool first) {
    Case<T> c(seed, k, cov);
    Stmt<T> s;
    if (dump) *dump << (first ? "" : ",\n") << "{\"seed\":" << seed << ",\"case\":" << k << ",\"type\":" << type_info_of<T>::id << ",\"class\":\"" << class_name(c.size_class) << "\",\"statements\":[";
    bool first_stmt = true;
    while (c.next(s)) {
        if (!dump) continue;
        *dump << (first_stmt ? "" : ",\n ");
        json_of(*dump, s);
        first_stmt = false;
    }
    if (dump) {
        *dump << "],\"pool\":";
        json_pool(*dump, c.model);
        *dump << "}";
    }
}

int main(int argc, char **argv) {
    std::uint64_t seed = 1, cases = 40;
    long long only = -1;
    int only_class = -1;
    const char *dump_path = nullptr;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const char *v = i + 1 < argc ? argv[i + 1] : "";
        if (a == "--seed") seed = std::strtoull(v, nullptr, 10), ++i;
        else if (a == "--cases") cases = std::strtoull(v, nullptr, 10), ++i;
        else if (a == "--case") only = std::atoll(v), ++i;
        else if (a == "--class") only_class = std::string(v) == "tiny" ? TINY : std::string(v) == "small" ? SMALL : MID, ++i;
        else if (a == "--dump") dump_path = v, ++i;
        else if (a == "--plan-only") continue;
        else {
            std::fprintf(stderr, "usage: surface_model_host --plan-only | --dump FILE  [--seed S] [--cases N] [--case K] [--class tiny|small|mid]\n");
            return 2;
        }
    }
    std::ofstream dump;
    if (dump_path) {
        dump.open(dump_path);
        dump << "[";
    }
    Coverage cov;
    bool first = true;
    for (std::uint64_t k = only >= 0 ? static_cast<std::uint64_t>(only) : 0; k < (only >= 0 ? static_cast<std::uint64_t>(only) + 1 : cases); ++k) {
        if (only_class >= 0 && class_of_case(k) != only_class) continue;
        std::ostream *out = dump_path ? &dump : nullptr;
        switch (type_of_case(k)) {
            case 0: run_case<float>(seed, k, cov, out, first); break;
            case 1: run_case<double>(seed, k, cov, out, first); break;
            case 2: run_case<int>(seed, k, cov, out, first); break;
            default: run_case<std::int64_t>(seed, k, cov, out, first); break;
        }
        first = false;
    }
    if (dump_path) dump << "]\n";
    cov.print(std::cout);
    std::printf("surface_model ok seed %llu\n", static_cast<unsigned long long>(seed));
    return 0;
}
