// stats.h -- annotation statistics used by the CVG/VCF writers (host side, scalar).
// Counterparts of /root/reference/src/Algorithm.cpp:9-67 (normsf, bt_fisher_exact, rankR1, RankSumTest).
// The reference takes kf_erfc and kt_fisher_exact from htslib's kfunc.c (SeqLib submodule, absent from the
// reference tree, version unpinned); both are restated here from the published algorithms.
#ifndef BVC_HOST_STATS_H
#define BVC_HOST_STATS_H

#include <cstddef>
#include <vector>

namespace bvchost {

double kf_erfc(double x);                                     // complementary error function (Hart, ~1e-15)
double kt_fisher_exact(int n11, int n12, int n21, int n22, double *left, double *right, double *two);

double normsf(double x);                                      // src/Algorithm.cpp:9-14
double bt_fisher_exact(int n11, int n12, int n21, int n22);   // src/Algorithm.cpp:16-25: phred of the two-sided p
double RankSumTest(std::vector<double> &x, std::vector<double> &y);   // src/Algorithm.cpp:55-67 (x is extended by y)
// The tail of RankSumTest (src/Algorithm.cpp:59-66): the phred-scaled two-sided p of the rank sum r1 of a first sample of n1 values
// among n1 + n2.  r1 may come from elsewhere: bvc_site_stats (include/bvc.h) carries 2 * r1 as an integer, and rank2 / 2.0 is the
// double rank_r1 returns.
double RankSumFromR1(double r1, size_t n1, size_t n2);

}  // namespace bvchost
#endif
