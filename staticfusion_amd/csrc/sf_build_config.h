// sf_build_config.h — the build axes of the device code, in one place: every macro the object table of the Makefile sets
// with -D, its default, what is derived from it, and which combinations are built. sf_device_common.h includes this first;
// no other file gives one of these macros a default or derives one from another. Three axes are "defined or not" (tested
// with #ifdef where they are used) and have no default: SF_CLUSTER, SF_NO_PROF_MARK, SF_KM_FINE_PROFILE.
//
// What the Makefile builds from sf_frame_kernels.hip (the host objects take every default):
//   object                     SF_NT  SF_OCC  SF_CLUSTER  SF_REFORDER  SF_FAST_WEIGHTS / SF_ROWS_FMA  other
//   frame_nt256[o5].o           256   4 [5]      -            0                  1 / 1
//   frame_nt1024.o             1024     4        -            0                  1 / 1
//   frame_cluster.o            1024     4       set           0                  1 / 1
//   frame_*_precise.o          the four above with                               0 / 0
//   frame_nt*_reforder.o       256 [o5], 1024    -            1                  0 / 0                SF_NO_PROF_MARK
//   frame_nt{256,1024}_kmprof.o  as frame_nt256.o / frame_nt1024.o                                    SF_KM_FINE_PROFILE
#pragma once

// threads per workgroup: 256 = the throughput variant (frame_nt256*.o), 1024 = latency and cluster (frame_nt1024*.o, frame_cluster*.o)
#ifndef SF_NT
#define SF_NT 256
#endif
// waves per SIMD the frame kernel is compiled for (__launch_bounds__): 4 = <= 128 VGPRs, 5 = <= 96 VGPRs (frame_nt256o5*.o)
#ifndef SF_OCC
#define SF_OCC 4
#endif
// SF_CLUSTER (defined or not): several 1024-thread workgroups per stream, sf_cluster.h (frame_cluster.o, frame_cluster_precise.o)
// the reference-order build, a parity instrument: the reference's float operation order everywhere, sf_reforder.h (frame_*_reforder.o)
#ifndef SF_REFORDER
#define SF_REFORDER 0
#endif
// per-pixel IRLS weights with the 1-ulp hardware rcp / rsq instead of IEEE division and square root; 0 in frame_*_precise.o, frame_*_reforder.o
#ifndef SF_FAST_WEIGHTS
#define SF_FAST_WEIGHTS 1
#endif
// rows and residuals of the IRLS passes contract multiply-add pairs explicitly (fmaf); 0 in frame_*_precise.o, frame_*_reforder.o
#ifndef SF_ROWS_FMA
#define SF_ROWS_FMA 1
#endif
// SF_NO_PROF_MARK (defined or not): no in-kernel stage timers inside the solve (frame_*_reforder.o)
// SF_KM_FINE_PROFILE (defined or not): timers inside the K-means chunk loop (frame_*_kmprof.o, `make kmprof`)
// levels of at most this many pixels take the ordered float splat in every build (sf_reforder.h); no Makefile object sets it
#ifndef SF_ORDERED_SPLAT_MAX_PIXELS
#define SF_ORDERED_SPLAT_MAX_PIXELS 2048  // (<= SF_CLUSTER_SOLO_PIXELS: a cluster's workgroups run such levels each on its own)
#endif

// ---- derived
// the linearisation walks register strips in the one-workgroup builds (solve_linearise_strips) and LDS tiles in a cluster,
// whose workgroups share a level tile by tile (solve_linearise)
#ifdef SF_CLUSTER
#define SF_LIN_STRIPS 0
#else
#define SF_LIN_STRIPS 1
#endif
// computeSegPrior rides in the strip sweep of the product builds; the reference-order build keeps ro_seg_prior
#define SF_LIN_FUSED_PRIOR (SF_LIN_STRIPS && !SF_REFORDER)
// pass 1 folds each row's pre-weight into its Cauchy weight (one reciprocal square root per row instead of two): part of the
// product build's arithmetic, off in the `precise` build, which keeps the reference's two-step association
#define SF_P1_FOLD (SF_FAST_WEIGHTS && SF_ROWS_FMA)
// workgroups per CU: 16 waves per CU at <= 128 VGPRs (5 x 256 per CU measured 3 % slower without segmentation: DESIGN.md §9)
#define SF_BLOCKS_PER_CU (SF_OCC * 256 / SF_NT)

// ---- the combinations that are not built are refused
#if SF_NT != 256 && SF_NT != 1024
#error "SF_NT must be 256 or 1024"
#endif
#if SF_OCC * 256 < SF_NT
#error "SF_OCC: fewer waves per SIMD than one workgroup of SF_NT threads needs"
#endif
#if defined(SF_CLUSTER) && !(SF_CLUSTER + 0)
#error "SF_CLUSTER is tested with #ifdef: leave it undefined instead of setting it to 0"
#endif
#if defined(SF_CLUSTER) && SF_REFORDER
#error "SF_CLUSTER and SF_REFORDER exclude each other: the reference-order build is one workgroup per stream (sf_create_ex refuses the cluster variant of libsf_hip_reforder.so, which links frame_cluster_precise.o)"
#endif
#if defined(SF_CLUSTER) && SF_NT != 1024
#error "SF_CLUSTER needs SF_NT=1024: one 1024-thread workgroup per CU (sf_cluster.h)"
#endif
#if SF_REFORDER && (SF_FAST_WEIGHTS || SF_ROWS_FMA)
#error "SF_REFORDER needs SF_FAST_WEIGHTS=0 and SF_ROWS_FMA=0: IEEE weights and no fmaf are part of the reference's order"
#endif
