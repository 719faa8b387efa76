// store_windows_main.cpp -- the position windows of --tmp-format mem (store_windows and store_window_ranges of host/pileup.cpp) and the
// parsing of their knob (parse_store_windows, store_windows_refused and auto_store_windows of host/knobs.h), for a build with
// -fsanitize=address,undefined (tests/test_store_windows.py builds this program and runs it).  Every array is a heap block of exactly the
// size the functions are told, so that a write or read past a window's slot is caught.  Usage: store_windows_main <knob value>...
// Prints one line per value ("<value> -> <what parse_store_windows returns>") and "<n> cases, 0 wrong" for the arithmetic.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "knobs.h"
#include "pileup.h"

using namespace bvchost;

int main(int argc, char **argv)
{
    for (int i = 1; i < argc; ++i) std::printf("%s -> %d\n", argv[i], parse_store_windows(argv[i]));
    std::printf("(unset) -> %d\n", parse_store_windows(nullptr));
    long cases = 0, wrong = 0;
    const size_t psizes[] = {0, 1, 5, 64, 1000, 66615};
    const int threads[] = {1, 2, 4, 8}, windows[] = {1, 2, 3, 7, 100, 8192};
    for (size_t psize : psizes)
        for (int T : threads)
            for (int K : windows) {
                ++cases;
                if (store_windows_refused(K, T)) { ++wrong; continue; }
                std::unique_ptr<size_t[]> a(new size_t[K]), b(new size_t[K]);
                std::unique_ptr<int32_t[]> wbeg(new int32_t[K]), wend(new int32_t[K]), pv(new int32_t[psize ? psize : 1]);
                std::unique_ptr<uint32_t[]> rec_start(new uint32_t[psize + 1]);
                for (size_t t = 0; t < psize; ++t) pv[t] = 5000 + 3 * (int32_t)t;          // 1-based positions, every third coordinate
                for (size_t t = 0; t <= psize; ++t) rec_start[t] = (uint32_t)(13 * t);
                store_windows(psize, T, K, a.get(), b.get());
                const int32_t beg0 = 3999, end0 = 5000 + 3 * (int32_t)psize + 1000;
                store_window_ranges(pv.get(), K, a.get(), b.get(), beg0, end0, wbeg.get(), wend.get());
                bool ok = a[0] == 0 && b[K - 1] == psize && wbeg[0] == beg0;
                int32_t reach = beg0;
                for (int w = 0; w < K; ++w) {
                    size_t lo, hi, lo2, hi2;
                    thread_window(psize, T * K, w * T, lo, hi);
                    thread_window(psize, T * K, w * T + T - 1, lo2, hi2);
                    ok = ok && a[w] == lo && b[w] == hi2 && a[w] <= b[w] && (w == 0 || a[w] == b[w - 1]);
                    ok = ok && wbeg[w] == reach && wend[w] >= wbeg[w];
                    // a window's positions lie inside the range its blocks are gathered for (the reads' filter is the region's beg0: the
                    // ranges say where gathering starts and stops, not which reads are kept)
                    if (a[w] < b[w]) ok = ok && wbeg[w] <= pv[a[w]] - 1 && pv[b[w] - 1] - 1 < wend[w];
                    reach = wend[w];
                }
                ok = ok && reach == end0;
                // auto: every K it returns is one the program takes, and a budget that holds the whole estimate asks for one window
                const int max_k = kStoreWindowsMaxThreads / T;
                const int k_small = auto_store_windows(rec_start.get(), psize, T, max_k, 4.0, 3, 20000.0);
                const int k_whole = auto_store_windows(rec_start.get(), psize, T, max_k, 4.0, 3, 1e12);
                ok = ok && k_small >= 1 && k_small <= max_k && k_whole == 1 && !store_windows_refused(k_small, T);
                if (!ok) { ++wrong; std::printf("wrong: psize %zu T %d K %d\n", psize, T, K); }
            }
    std::printf("%ld cases, %ld wrong\n", cases, wrong);
    return wrong ? 1 : 0;
}
