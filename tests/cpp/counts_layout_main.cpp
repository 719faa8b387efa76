// counts_layout_main.cpp -- csrc/counts_layout.h alone in a stand-alone program (tests/test_bam_counts_quals_abi.py builds it with
// -fsanitize=address,undefined and compares every line with the models and the headers' closed forms).  One line a case:
//   kind n_groups n_quals -> count_words logical_words bytes_per_position expanded label_groups
// and one line `quals_ok` with the values of -4..139 that pass.
#include <cstdio>

#include "counts_layout.h"

using bvc::CountsLayout;

static void line(const char *kind, int n_groups, int n_quals, const CountsLayout &l)
{
    std::printf("%s %d %d -> %zu %zu %zu %d %u\n", kind, n_groups, n_quals, l.count_words(), l.logical_words(), l.bytes_per_position(), (int)l.expanded(),
                l.label_groups());
}

int main()
{
    const int wide_groups[] = {0, 1, 5, 32}, depth_groups[] = {1, 5, 32}, quals[] = {4, 40, 124, 128}, narrow_groups[] = {0, 5, 32};
    for (int g : wide_groups) line("wide", g, 128, CountsLayout::wide(g));
    for (int g : depth_groups) line("with_depth", g, 128, CountsLayout::with_depth(g));
    for (int q : quals)
        for (int g : narrow_groups) line("narrow", g, q, CountsLayout::narrow(q, g));
    std::printf("quals_ok");
    for (int q = -4; q <= 139; ++q)
        if (CountsLayout::quals_ok(q)) std::printf(" %d", q);
    std::printf("\n");
    return 0;
}
