/*
 * mi_icp_debug.h -- test-only entry points of libmi_icp.so.  Not part of the
 * drop-in boundary (nothing in the reference binds to these): they expose the
 * hand-written device primitives (radix sort, exclusive scan) that replace
 * thrust::sort_by_key / exclusive_scan inside the engine, so that the parity
 * tests can pin them on their own.  Buffers are host memory.
 * (and the built tree, for invariant tests)
 */
#ifndef MI_ICP_DEBUG_H_
#define MI_ICP_DEBUG_H_
#include "mi_icp.h"
#ifdef __cplusplus
extern "C" {
#endif
/* stable LSD radix sort of (key, value) pairs by the low key_bits bits, in place */
MI_ICP_API int mi_icp_debug_sort_pairs(mi_icp_ctx* ctx, uint64_t* keys, uint32_t* vals,
                                       int64_t n, int key_bits);
/* the same sort in its narrow form (32-bit keys: radix_sort_pairs<uint32_t>), key_bits 1 .. 32 */
MI_ICP_API int mi_icp_debug_sort_pairs32(mi_icp_ctx* ctx, uint32_t* keys, uint32_t* vals,
                                         int64_t n, int key_bits);
/* the payload form (radix_sort_payload32): 32-bit keys sorted stably on the bits [lo_bit, hi_bit), up to three arrays
 * of n * 3 floats (NULL: absent) travelling with them; keys and the present arrays are sorted in place.
 * 0 <= lo_bit <= hi_bit <= 32, else MI_ICP_ERR_INVALID; lo_bit == hi_bit is no pass: the input comes back unchanged. */
MI_ICP_API int mi_icp_debug_sort_payload32(mi_icp_ctx* ctx, uint32_t* keys, float* a0, float* a1, float* a2,
                                           int64_t n, int lo_bit, int hi_bit);
/* What the sort drivers choose for n >= 1 elements, from the drivers' own tables (csrc/primitives.h; no context, no GPU
 * call): out[0] = 1 if the pair sort takes its one-launch path (tiles of 2048, whatever [1] and [2] say), [1] = the
 * pair tiers' 64-element chunks per wave (a tile is 512 * chunks elements), [2] = the tiles of that size in n,
 * [3], [4] = the same of the payload sort, [5] = sort_hist_segments(n): the histogram segments a buffer set for n
 * holds, for every sort of m <= n elements, [6] = scan_num_tiles(256 * [5]), [7] = 0. */
MI_ICP_API int mi_icp_debug_sort_plan(int64_t n, int32_t out[8]);
/* out[i] = sum of in[0..i); *total = sum of all (out may alias in) */
MI_ICP_API int mi_icp_debug_exclusive_scan(mi_icp_ctx* ctx, const uint32_t* in, uint32_t* out,
                                           int64_t n, uint64_t* total);
/* Morton order of a cloud as the engine computes it: order[sorted] = original */
MI_ICP_API int mi_icp_debug_morton_order(mi_icp_ctx* ctx, const float* xyz, int64_t n,
                                         uint32_t* order);
/* The same order on the cloud's own bounds with a grid of 2^bits cells per axis given from outside (bits 1 .. 21:
 * morton_order's grid_bits form).  The engine's own choice of bits stays at or below 10
 * (32-bit keys) for every cloud below 2^30 points; 3 * bits > 32 runs the 64-bit keys and their sort. */
MI_ICP_API int mi_icp_debug_morton_order_bits(mi_icp_ctx* ctx, const float* xyz, int64_t n, int bits,
                                              uint32_t* order);
/* traversal census of one nearest-neighbour pass: out4 = {node visits summed over
 * packets, leaf visits, packets, visits (nodes + leaves) of the slowest packet}.
 * use_seed != 0 seeds from the previous pass. */
MI_ICP_API int mi_icp_debug_nn_stats(mi_icp_ctx* ctx, const float* T, float radius, int use_seed,
                                     uint64_t* out4);
/* the same pass with four more counters: out8[4] = halo lines evaluated (leaf_halo.h), [5] = packets
 * that evaluated any, [6] = packets that walked the tree, [7] = lanes unfinished when their packet's walk
 * started. */
MI_ICP_API int mi_icp_debug_nn_stats8(mi_icp_ctx* ctx, const float* T, float radius, int use_seed,
                                      uint64_t* out8);
/* Forget the previous search result: the next nearest-neighbour pass starts top-down instead of
 * from its predecessor's matches (tests compare the two; the results must be identical).  The
 * context has no correspondence set until that pass has run. */
MI_ICP_API int mi_icp_debug_drop_seeds(mi_icp_ctx* ctx);
/* How the last nearest-neighbour pass started: 0 = from the root (no previous matches), 1 = from the
 * previous pass's matches, 2 = from seeds it made itself (a greedy descent per query; what a registration
 * loop's first pass does when the target's halos exist already), -1 = no pass yet. */
MI_ICP_API int mi_icp_debug_last_search_kind(const mi_icp_ctx* ctx);
/* Which path the last mi_icp_voxel_downsample call took: 1 = the dense-grid path (csrc/voxel_dense.h: one partition,
 * a workgroup per bucket), 0 = the general path (radix passes with the payload), -1 = no call yet (or one that returned
 * early: an empty cloud, a voxel size <= 0, a grid beyond int32).  Both are exact; tests run each on purpose
 * (the switch MI_ICP_NO_DENSE_VOXEL is read at every call). */
MI_ICP_API int mi_icp_debug_last_voxel_path(const mi_icp_ctx* ctx);
/* What the last mi_icp_voxel_downsample call ran, as the host decided it (csrc/mi_voxel.hip; no launch, no wait):
 * out[0] = the path as above (-1 / 0 / 1), [1] = the packed key's bits (x + y + z), [2] = L (the low key bits left
 * unsorted), [3] = sort passes, [4] = sort kind (0 none, 1 payload radix of 8-bit digits, 2 wide sort of 11-bit digits,
 * 3 64-bit (key, index) pairs, 4 three sorts, one per axis), [5] = means kernel (0 vx_finish of the dense path,
 * 1 voxel_means_wave, 2 voxel_means_runs, 3 voxel_means_thread, 4 voxel_means), [6] = voxels written, [7] = 0.
 * The dense path sorts nothing: [2] .. [5] are 0 there.  A call that returned early leaves [1] .. [7] zero. */
MI_ICP_API int mi_icp_debug_last_voxel_plan(const mi_icp_ctx* ctx, int32_t out[8]);
/* Resident workgroups per CU the runtime grants a kernel at its launch shape (hipOccupancyMaxActiveBlocksPerMultiprocessor):
 * which = 0 kd_build_groups, 1 nn_packet_kernel<seeded>, 2 nn_packet_kernel<from the root>, 3 reduce_pt2pl_kernel<2,1> with the pair stream,
 * 4 leaf_halo_build, 5 rs_scatter_pay<8>, 6 voxel_means_wave, 7 vx_scatter<1>, 8 vx_finish<points only>,
 * 9 reduce_pt2pl_kernel<4,1> with the pair stream (sources below 4 Mi points; 3 is the instantiation of larger ones; until
 * the pair stream 3 was the plain <2,1>).  The reductions are launched two workgroups per CU.  Returns the count, < 0 on error. */
MI_ICP_API int mi_icp_debug_occupancy(int which);
/* Where an iteration's time goes (csrc/loop.h): with stamps enabled the NEXT registration loop on the context runs the
 * same search / point-to-plane reduction kernels instantiated with device-clock stamps (s_memrealtime, one clock for the
 * whole GPU): the search's first wave start / last wave end, the reduction's first block start, the last block's
 * ticket, rows totalled, ranks' exchange done, solve done, state written.  get: the 32 stamp words -- [0..7] the
 * current iteration's stamps (re-armed), [16..23] the SUMS of the eight spans over the iterations counted in [24]:
 * step-end -> next search start, search, search end -> reduction start, reduction's streaming phase, row total,
 * exchange, solve, state write -- and the clock's ticks per microsecond. */
/* Counters of the present registration loop as of its last host-side look: out4 = {iterations (updates applied),
 * passes (evaluations), re-locations (steps that moved the source by more than about a leaf's width, ~1.9 point spacings, and had the next
 * search's seeds replaced by the leaves the moved queries fall into: csrc/loop.h, nn_search.h locate_by_planes),
 * 1 if the next chunk of iterations would still carry the gated re-location launches}. */
MI_ICP_API int mi_icp_debug_loop_counters(mi_icp_ctx* ctx, int32_t* out4);
/* The search skip's state (csrc/nn_search.h "the skip", csrc/loop.h) of the present registration loop, large sources
 * only: state2 = {the loop's odometer `travel`, the present bound `fuzz` on the queries' rounding}, *npackets = the
 * source's packets of 64 points, limits_out[packet] (host memory, filled when capacity >= *npackets; may be NULL) = the
 * limit the packet's last search left (-inf or NaN: none), *armed = 1 if the loop's next search will be gated at all (the
 * limits on record belong to its radius, nothing has voided them since, and by the loop state's sample at least a
 * quarter of the packets hold one: csrc/loop_policy.h skip_pays).  That search skips exactly the packets with
 * travel + fuzz < limit, travel and fuzz as its own step leaves them.  Fails without a loop. */
MI_ICP_API int mi_icp_debug_search_skip(mi_icp_ctx* ctx, double* state2, double* limits_out, int64_t capacity,
                                        int64_t* npackets, int* armed);
/* The pair stream's state (csrc/reduce.h PairArgs) as the last launch left it: *n_out = the staged source's
 * packets of 64 points; state_out[packet] (one byte each: 0 a match changed in the last search or nothing is known, 1 the
 * reduction has seen the packet once since, 2 its record of matched points and normals is valid) and mask_out[packet] (bit l:
 * lane l exists and has a match; meaningful in state 2) are host memory, filled when capacity >= *n_out; either may be NULL.
 * Fails without a staged source. */
MI_ICP_API int mi_icp_debug_pair_state(mi_icp_ctx* ctx, uint8_t* state_out, uint64_t* mask_out, int64_t capacity,
                                       int64_t* n_out);
/* Every packet's pair state back to 0 -- and nothing else: matches, limits of the search skip and the loop stay.  The
 * next two reductions of a loop gather every record again (tests compare that path with the pair stream's: the results
 * must be identical bit for bit). */
MI_ICP_API int mi_icp_debug_drop_pairs(mi_icp_ctx* ctx);
/* The leaf every staged source point FALLS INTO under T (column-major 4x4 or NULL) by the binary descent through the
 * cell planes and its group's planes (nn_search.h locate_by_planes): leaf_out[original source index] = leaf (host memory,
 * one per source point).  The located leaves are left behind as the seeds of the next seeded pass.  Fails without a
 * staged source and target. */
MI_ICP_API int mi_icp_debug_locate(mi_icp_ctx* ctx, const float* T, int32_t* leaf_out);
MI_ICP_API int mi_icp_debug_set_step_stamps(mi_icp_ctx* ctx, int enable);
MI_ICP_API int mi_icp_debug_get_step_stamps(mi_icp_ctx* ctx, uint64_t* out32, double* ticks_per_us);
/* The loop step's two forms of utility::SolveJacobianSystemAndObtainExtrinsicMatrix side by side, on the
 * device: n systems of 32 doubles each (host memory; the reduction's layout: 21 upper-triangle sums of
 * JtJ, 6 of Jtr, ...) are solved by one thread with the serial routines and by a wave with a matrix row
 * per lane.  out_serial / out_wave: n * 16 floats (column-major 4x4); ok_serial / ok_wave: n flags
 * (0 = the determinant check failed, result identity).  The two must agree bit for bit. */
MI_ICP_API int mi_icp_debug_solve_both(int device, const double* systems, int n, float det_thresh,
                                       float* out_serial, float* out_wave, int32_t* ok_serial, int32_t* ok_wave);
/* csrc/eigen3.h one matrix at a time, so that an outside implementation (LAPACK through numpy, in fp64) can be held
 * against it: n symmetric 3x3 matrices A (row-major, host memory) -> eval (n * 3), evec (n * 9 row-major, COLUMN k =
 * eigenvector k), S (n * 9: what the GICP reduction adds for W = SqrtMatrix3x3(A), S = W W) as FastEigen3x3 /
 * gicp_weight compute them -- on the host (device < 0: the __host__ half of the same functions, no GPU needed) or in
 * a kernel on that device (the GPU's own acosf / cosf / sqrtf / divisions).  Any output may be NULL. */
MI_ICP_API int mi_icp_debug_eigen3(int device, const float* A, int64_t n, float* eval, float* evec, float* S);
/* One image of the LAST mi_icp_compute_[weighted_]rgbd_odometry call on the context, as its iterations read it: level
 * 0 .. num_levels - 1 (0 = full size), which = 0 source colour, 1 source depth, 2 target colour, 3 target depth (Gaussian3,
 * invalid depth NaN, colour scaled by NormalizeIntensity, downsampled per level), 4 dx colour, 5 dy colour, 6 dx depth,
 * 7 dy depth (Sobel3Dx / Sobel3Dy of the target, unscaled).  *width x *height floats to out (host memory; NULL: the size
 * only).  The images live in a scratch buffer that other entry points reuse: valid only DIRECTLY after the odometry
 * call, before anything else runs on the context.  MI_ICP_ERR_INVALID when no odometry call has completed on the
 * context or level / which is out of range. */
MI_ICP_API int mi_icp_debug_odometry_image(mi_icp_ctx* ctx, int level, int which, float* out, int* width, int* height);
/* The target's tree as built by mi_icp_set_target, for invariant tests.  info5 = {slots
 * (padded sorted positions), leaves, leaf_first (id of the first leaf-level node), records,
 * points}.  records_out (records * 64 floats: 8 child boxes as 4 sibling pairs of 12,
 * floats 48..53 the node's region, 54 its validity flag) and leaf_lines_out (leaves * 32
 * floats: x[8] y[8] z[8] original index[8], padding = +inf / -1; on the device a line's fourth
 * row holds the leaf's region record and the indices are an array of their own -- the export
 * puts the indices there) may be NULL to query the sizes only. */
MI_ICP_API int mi_icp_debug_get_tree(mi_icp_ctx* ctx, int64_t* info5, float* records_out,
                                     float* leaf_lines_out);
/* Per leaf (mi_icp_debug_get_tree's info5[1] leaves) 8 floats: region lo.xyz, word A, region hi.xyz,
 * word B.  The region is free of points of any other leaf (an invalid one is +inf / -inf: nothing is
 * inside).  Words A and B pack the reaches of the leaf's eight halo lines as 6-bit fractions of the bound:
 * A = q0 .. q4 (6 bits each from bit 0), bits 30-31 the low two bits of q7; B = q5 (bits 0-5), q6 (6-11),
 * the high four bits of q7 (12-15), the bound (the upper 16 bits of an fp32) on top; reach k = bound / 64 *
 * q_k.  B = 0: no halo. */
MI_ICP_API int mi_icp_debug_get_leaf_regions(mi_icp_ctx* ctx, float* regions_out);
/* Per leaf 8 halo lines of 32 floats (builds them if no seeded search has yet): x[8] y[8] z[8] slot[8] --
 * line k holds the points of OTHER leaves that are 8k+1-th .. 8k+8-th nearest to the leaf's region
 * (L-infinity distance to the box), ascending in slot (sorted target position, as an integer's bits; unused
 * entries +inf / -1).  Every point of another leaf nearer to the region than reach k is in the lines 0 .. k.
 * Call mi_icp_debug_get_leaf_regions afterwards for the regions and reaches. */
MI_ICP_API int mi_icp_debug_get_leaf_halos(mi_icp_ctx* ctx, float* halos_out);
/* mi_icp_image_bilateral with the exponential named: exp_kind 1 the hardware 2^x of arg * log2(e) (what
 * mi_icp_image_bilateral runs), 0 the library's expf.  For scripts/dev/image_rows.py, which times both, and for the
 * test that holds both to the same bound. */
MI_ICP_API int mi_icp_debug_image_bilateral(mi_icp_ctx* ctx, const float* src, int width, int height, int diameter,
                                            float sigma_color, const float* table, float* dst, int exp_kind);
#ifdef __cplusplus
}
#endif
#endif
