/* mickey_hip_dev.h -- development knobs of libmickey_hip.so (benchmarks, tests, A/B tools).
 *
 * NOT part of the drop-in ABI (include/mickey_hip.h): these set PROCESS-WIDE state that selects between kernel
 * schedules computing the same result.  The product path never calls them.
 */
#ifndef MICKEY_HIP_DEV_H
#define MICKEY_HIP_DEV_H

#ifdef __cplusplus
extern "C" {
#endif

/* Schedule of the GEMM / implicit-GEMM conv kernel: 0 = automatic (128x128 tiles for small problems, the default
 * 256x256 schedule for large ones; 64x128 tiles where 128x128 would leave CUs idle), 1 = force 128x128 (4 waves, 2
 * workgroups per CU), 2 = force 64x128 (same kernel, half the rows, 3 LDS stages), 7 = force the
 * 8-wave ping-pong 256x256 schedule (two waves per SIMD);
 * 400 + b sets the band height b (in m-tiles) of the 256x256 tile order, 464 + g walks groups of g n-tiles m-major instead
 * (400 / 464: automatic = n-fastest for outputs <= 4 tiles wide, bands of 8 otherwise); 500 / 501 switch the automatic use of the 64x128
 * tiling off / on; 600 / 601 / 602: the persistent tile loop of the 256x256 kernel (one workgroup per CU walking a continuous K stream over
 * its tiles, the next tile's first operands in flight under the current epilogue) wherever it applies (consumers qkv / fc1 too) / off /
 * for the producers proj, fc2, patch embed only (default: the measured best, profiles/r06u_persist_ab.txt). */
int mk_gemm_set_tile(int mode);

/* Kernel variant of mk_flash_attn_fwd: 0 = automatic (2 for >= 512 workgroups of 256 queries, 1 for smaller grids),
 * 1 / 2 = the production kernel with 32 / 64 queries per wave (lean softmax: running maximum folded into the MFMA
 * accumulator init, re-based only when a tile outgrows it, seen in the row sums; fp32 row sums on the VALU), 3 = the classic online-softmax
 * kernel (64 queries per wave; A/B partner), 4 / 5 = the production kernel's structure on v_mfma_f32_16x16x32 instead of
 * 32x32x16 (32 / 64 queries per wave): +3-5 % at 32 pairs, the cheaper shape per flop at the power limit, 12-17 % slower for
 * one pair; 6 = 2 without the one-sub-block tail wave (round 6's A/B partner, profiles/r06r_attn_padding_skips.txt); 1 / 2 / 6 and
 * 4 / 5 are each bit-identical families, the two families differ in the last bits.  Process-wide; for benchmarks and tests. */
int mk_attn_set_mode(int mode);

/* Measurement probe (bench.py `roofline.peak_sustained`): back-to-back v_mfma_f32_16x16x32 (bf16) on register-resident operands
 * (pseudo-random, or zeros), `workgroups` x 8 waves x `iters` x 8 MFMAs = workgroups * iters * 1048576 flops per launch, no memory
 * traffic: what the socket power limit lets through the matrix pipe alone (LABNOTES R4.11).  scratch: >= workgroups * 512 floats. */
int mk_dev_mfma_sustained(float* scratch, int workgroups, int iters, int zero_operands, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MICKEY_HIP_DEV_H */
