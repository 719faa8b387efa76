// counts_layout.h -- the one description of a kind of class-count accumulator (include/bvc_bam_counts.h, bvc_bam_group_depth.h,
// bvc_site_acc_quals.h, bvc_site_acc_pack.h): how a position's counts are stored, what lies beside them, and every size that follows.
// Plain C++11 with no HIP dependence (tests/cpp/counts_layout_main.cpp compiles it alone); bvc_internal.h includes it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bvc {

// Which instantiation of bam_counts_kernel adds into a layout
enum class CountsKind { Slots, Depth, Narrow };

// The rows a launch of acc_pack_kernel.hip's kernels works on: row0 is the first of them in the accumulator's arrays, count_pieces the
// 16-byte pieces of a position's counts as they are STORED, q4 = n_quals / 4 for narrow rows (0: the wide layout), count_cells the LOGICAL
// count cells (slots x 512).
struct AccRowShape { int64_t row0; uint32_t count_pieces, q4, count_cells, depth_groups; };

struct CountsLayout {
    uint32_t slots;                                 // slots of counts a position: n_groups + 1 where every group has its own, else 1
    uint32_t n_quals;                               // quality columns stored per base; 128: wide rows [slots][512]
    uint32_t depth_groups;                          // groups whose depths per base [depth_groups][4] lie beside ONE slot of counts

    // counts [P][slots][512], a slot per group and one for the samples in none (bvc_bam_counts, bvc_site_acc_create)
    static CountsLayout wide(int32_t n_groups) { return CountsLayout{n_groups > 0 ? (uint32_t)n_groups + 1u : 1u, 128u, 0u}; }
    // counts [P][512] and group_depth [P][n_groups][4] (bvc_bam_counts_depth, bvc_site_acc_create_depth)
    static CountsLayout with_depth(int32_t n_groups) { return CountsLayout{1u, 128u, (uint32_t)n_groups}; }
    // counts [P][4][n_quals] and, with groups, group_depth (bvc_bam_counts_quals, bvc_site_acc_create_quals); 128 columns are wide rows
    static CountsLayout narrow(int32_t n_quals, int32_t n_groups) { return CountsLayout{1u, (uint32_t)n_quals, (uint32_t)n_groups}; }

    static bool quals_ok(int32_t n_quals) { return n_quals >= 4 && n_quals <= 128 && n_quals % 4 == 0; }
    bool quals_ok() const { return quals_ok((int32_t)n_quals); }

    bool expanded() const { return n_quals < 128u; }                     // its rows are not the [512] layout: acc_expand_kernel makes it
    CountsKind kind() const { return expanded() ? CountsKind::Narrow : depth_groups > 0u ? CountsKind::Depth : CountsKind::Slots; }
    // the groups a sample's label is compared with; > 0: group_of_sample is read
    uint32_t label_groups() const { return slots > 1u ? slots - 1u : depth_groups; }
    size_t count_words() const { return (size_t)slots * 4 * n_quals; }   // stored words of counts a position
    size_t logical_words() const { return (size_t)slots * 512 + 10 + (size_t)depth_groups * 4; }       // W of bvc_site_acc_pack.h
    size_t bytes_per_position() const { return count_words() * 4 + 48 + (size_t)depth_groups * 16; }    // counts, tally, depths
    AccRowShape row_shape(int64_t row0) const
    {
        return AccRowShape{row0, (uint32_t)(count_words() / 4), expanded() ? n_quals / 4u : 0u, slots * 512u, depth_groups};
    }
};

}  // namespace bvc
