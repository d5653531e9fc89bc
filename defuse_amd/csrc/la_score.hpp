// la_score.hpp — scores against a percent-perfect threshold (tools/localalign.cpp:84-92, tools/matealign.cpp:191-201), the one
// definition for the tools (tools_src/defuse_host.hpp) and for conc_api.hip.  Plain host C++.
// maxScore = len(sequence) * match (a size_t product stored in an int), percent = (double) score / maxScore, and a line is printed
// unless percent < threshold.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

inline int score_max(size_t seq_len, int matchScore) { return (int)(seq_len * (size_t)matchScore); }

// the smallest score a line needs to be printed at all: below it the device may stop early (la_align_batch_min's min_score)
inline int32_t threshold_min_score(int maxScore, double threshold)
{
    int32_t s = std::numeric_limits<int32_t>::min();
    if (maxScore > 0 && threshold > 0.0) {
        s = (int32_t)std::min<double>(std::ceil(threshold * (double)maxScore), 2147483000.0);
        while (s > 0 && !((double)(s - 1) / (double)maxScore < threshold)) --s;     // exactly the test of the line filter
        while ((double)s / (double)maxScore < threshold) ++s;
    }
    return s;
}
