// syncruns_main.cpp -- stand-alone driver of syncruns.cpp, for a build with -fsanitize=address,undefined: every file
// named on the command line through probe_sync_runs at R = 1, 2, 4 and 128- / 256-byte subsequences, every scan.
// Prints one line per run; exit status 1 if a run leaves an entry unset, wrong after the tail's rule, or marked inside a run.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int probe_sync_runs(const uint8_t* data, size_t size, int subseq_bytes, int scan, int R, long long* out);

int main(int argc, char** argv)
{
    int failures = 0;
    for (int a = 1; a < argc; ++a) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> data;
        uint8_t buf[65536];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + n);
        std::fclose(f);
        for (int bytes : {128, 256})
            for (int R : {1, 2, 4})
                for (int scan = 0;; ++scan) {
                    long long out[24] = {};
                    const int rc = probe_sync_runs(data.data(), data.size(), bytes, scan, R, out);
                    if (rc == -1 && scan > 0) break; // no such scan
                    const bool ok = rc == 0 && out[7] == 0 && out[10] == 0 && out[6] == 0 && (R != 1 || out[8] == 0);
                    std::printf("%s bytes=%d R=%d scan=%d rc=%d S=%lld spec=%lld flow=%lld marks=%lld wrong_after_tail=%lld %s\n", argv[a], bytes, R,
                        scan, rc, out[0], out[2], out[3], out[5], out[7], ok ? "ok" : "FAILED");
                    failures += !ok;
                    if (rc != 0) break;
                }
    }
    return failures ? 1 : 0;
}
