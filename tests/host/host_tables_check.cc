// Stand-alone walk over the engine's host-only units (ctucopy_amd/csrc/accept.cc, tables.cc with opts.cc and design.cc): no engine
// library, no GPU, no HIP.  tests/test_host_tables.py builds it under Address+UB sanitizers and runs it on the configurations of
// tests/golden/host_tables.json: exit status 0, a silent stderr and the golden file's hashes and refusal texts are the result.
//
// Input (argv[1]), a line per configuration, tab-separated:  kind  name  flags  arg...
//   kind T: the "host_tables" report (ctu::host_tables_report)   -> T name <values> <sha256 of the values as little-endian float64>
//   kind C: what ctu_engine_create answers ahead of the device   -> R name <code> <text in hex>
//   kind S: ctu_streams_config_check_ex with `flags`             -> R name <code> <text in hex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "accept.h"
#include "check_digest.h"
#include "tables.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    int n = 0;
    while (std::getline(in, line)) {
        std::vector<std::string> f;
        std::stringstream ss(line);
        for (std::string t; std::getline(ss, t, '\t');) f.push_back(t);
        if (f.size() < 3) return 2;
        const std::string kind = f[0], name = f[1];
        const uint32_t flags = (uint32_t)std::stoul(f[2]);
        const std::vector<std::string> args(f.begin() + 3, f.end());
        int code = CTU_OK;
        std::string text;
        try {
            ctu::Design d(ctu::Opts::from_args(args));
            if (kind == "T") {
                const std::vector<double> v = ctu::host_tables_report(d);  // (x86-64: a double in memory is its little-endian float64)
                std::printf("T %s %zu %s\n", name.c_str(), v.size(), sha256(reinterpret_cast<const unsigned char *>(v.data()), v.size() * sizeof(double)).c_str());
                n++;
                continue;
            }
            ctu::spread_small_fft(d);
            code = kind == "S" ? ctu::streams_check(d, flags, text) : ctu::create_check(d, text);
        } catch (const std::exception &ex) {  // as ctu_engine_create / ctu_streams_config_check_ex answer what the parser or the design throws
            code = CTU_ERR_OPTS;
            text = ex.what();
        }
        std::printf("R %s %d %s\n", name.c_str(), code, hex(text).c_str());
        n++;
    }
    std::printf("host_tables_check ok: %d configurations\n", n);
    return 0;
}
