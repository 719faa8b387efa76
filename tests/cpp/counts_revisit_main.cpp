// counts_revisit_main.cpp -- the revisit rule of a run that piles phase 1 into class counts (counts_revisit of host/pileup.h), for a build with
// -fsanitize=address,undefined (tests/test_counts_revisit.py builds this program and runs it).  Every array is a heap block of exactly the
// size the function is told, so that a flag set past a window's end -- or a predecessor looked for in front of its start -- is caught.
// The rule is held to a second statement of it, position by position: a flag set is the union of "called", "has indel entries" and "some
// indel position of my window follows me with no base token in between".  Prints "<n> cases, 0 wrong".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "pileup.h"

using namespace bvchost;

static uint32_t next_word(uint64_t &state)
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}

int main()
{
    long cases = 0, wrong = 0;
    const size_t psizes[] = {0, 1, 2, 5, 64, 1000, 6661};
    const int threads[] = {1, 2, 4, 8, 13};
    uint64_t state = 20261020;
    for (size_t psize : psizes)
        for (int T : threads)
            for (int density = 0; density < 3; ++density) {
                ++cases;
                std::unique_ptr<bvc_bam_site_tally[]> tally(new bvc_bam_site_tally[psize]);
                std::unique_ptr<uint8_t[]> called(new uint8_t[psize]), flags(new uint8_t[psize]);
                std::memset(flags.get(), 0xEE, psize);
                for (size_t t = 0; t < psize; ++t) {
                    std::memset(&tally[t], 0, sizeof tally[t]);
                    const uint32_t r = next_word(state);
                    const uint32_t every = density == 0 ? 2 : density == 1 ? 7 : 50;
                    if (r % every == 0) tally[t].strand_base[(r >> 8) & 7] = 1 + ((r >> 12) & 3);
                    if ((r >> 16) % (3 * every) == 0) tally[t].n_other = 1;
                    if ((r >> 20) % 11 == 0) tally[t].n_indel = 1 + ((r >> 28) & 1);
                    called[t] = (r >> 24) % 29 == 0;
                }
                counts_revisit(tally.get(), called.get(), psize, T, flags.get());
                bool ok = true;
                for (int i = 0; i < T && ok; ++i) {
                    size_t lo, hi;
                    thread_window(psize, T, i, lo, hi);
                    for (size_t t = lo; t < hi && ok; ++t) {
                        uint64_t bases = tally[t].n_other;
                        for (int k = 0; k < 8; ++k) bases += tally[t].strand_base[k];
                        bool carry = false;                  // the next indel position of the window, with no base token in between
                        for (size_t u = t + 1; u < hi && bases > 0; ++u) {
                            if (tally[u].n_indel > 0) { carry = true; break; }
                            uint64_t b = tally[u].n_other;
                            for (int k = 0; k < 8; ++k) b += tally[u].strand_base[k];
                            if (b > 0) break;
                        }
                        const uint8_t want = (uint8_t)((called[t] ? kRevisitCalled : 0) | (tally[t].n_indel > 0 ? kRevisitIndel : 0) | (carry ? kRevisitCarry : 0));
                        ok = flags[t] == want;
                    }
                }
                if (!ok) { ++wrong; std::printf("wrong: psize %zu T %d density %d\n", psize, T, density); }
            }
    std::printf("%ld cases, %ld wrong\n", cases, wrong);
    return wrong ? 1 : 0;
}
