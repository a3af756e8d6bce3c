// sf_window_args.h — the table entry and the block size of the stable partition (kernels: sf_map_window.h), for those that
// fill ballots and block counts of their own and have the scan and the ordered write launched for them (sf_join.h,
// sf_body_maps.h through sfw_launch_scan / sfw_launch_write of sf_hip_map_window.hip). No kernel here.
#pragma once

#define SFW_BLOCK 256  // surfels per workgroup (SF_CLEAN_BLOCK's reasoning: a QVGA map still covers the CUs)
#define SFW_WAVES (SFW_BLOCK / 64)

struct WindowArgs {
    const float *src;  // count x 12 (the map's buf[0])
    float *dst;        // the map's idle buffer
    int count;
    int move_rest;     // 0: only the selected surfels are moved (cull, extract: nobody reads [k, count) of dst)
    // the filter (include/sf_map_window.h); a disabled test has use_* == 0
    int use_conf, use_age, use_radius, invert;
    float min_confidence;
    float tick, max_age;     // (float)tick of the map, (float)max_age
    float cx, cy, cz, r2;    // centre, radius * radius
    unsigned long long *ballots;  // [ceil(count / 64)]: bit l of word w = surfel 64 w + l is selected
    int *block_counts;            // [ceil(count / SFW_BLOCK)]: selected per block; the scan turns them into exclusive offsets
    int *result;                  // [0]: k, the number selected
};
