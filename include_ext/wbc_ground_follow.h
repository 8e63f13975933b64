/*
 * wbc_ground_follow.h -- C ABI of the follow law of the compliant-ground plant (libwbc_hip.so): the entry points that make the
 * controllers' targets follow the terrain set on a wbc_ground handle.  The law, its modes WBC_FOLLOW_OFF / _LIFT / _FIT and its
 * limits are defined at the head of include/wbc_ground.h ("Following the ground"); the conventions are that header's.
 *
 * These three prototypes have a header of their own, in a directory beside include/, because the set of prototypes that the headers of
 * include/ itself declare is pinned as it stands (tests/test_abi_cpu.py counts it); tests/test_follow_cpu.py holds this header to its binding table
 * (quadruped_drake_amd/_lib.py: EXT_PROTOTYPES) by the same rules.
 */
#ifndef WBC_GROUND_FOLLOW_H
#define WBC_GROUND_FOLLOW_H

#include "../include/wbc_ground.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The follow law in place on targets [54][ld], for the terrain set on the handle (its table, terrain_id and terrain_scale); only the
 * rows the law changes are written: the z rows of every usable foot and of the body, in WBC_FOLLOW_FIT also the nine attitude rows.
 * mode = WBC_FOLLOW_OFF, n = 0, or no terrain set: success, and nothing is launched.  < 0 with the message set, before any device
 * call, for a null handle, a mode outside 0 .. 2, n < 0 or n > WBC_MAX_LD, ld < n or ld > WBC_MAX_LD, or null targets with n > 0. */
int wbc_ground_follow_targets(wbc_ground g, void* hip_stream, int n, int ld, int mode, double* targets);
/* What wbc_ground_rollout does between its lookup and its tick: with a mode other than WBC_FOLLOW_OFF (the default) and a terrain set,
 * every tick runs lookup -> follow -> wbc_step -> ground step, and on return targets holds the last tick's followed targets.  With
 * WBC_FOLLOW_OFF or no terrain set the rollout issues exactly the launches it issues without this call. */
int wbc_ground_set_follow(wbc_ground g, int mode);
/* wbc_ground_kernel_info of the follow kernel. */
int wbc_ground_follow_kernel_info(wbc_ground g, int* num_vgpr, int* scratch_bytes, int* lds_bytes, int* block_threads);

#ifdef __cplusplus
}
#endif
#endif
