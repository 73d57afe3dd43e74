/* The optimiser extension of libgcgcn_hip.so: Adam with weight decay (L2 or decoupled), amsgrad, maximize, bias correction
 * switched off, and ONE clipping norm over all parameter groups (csrc/optim.hip; gcgcn_amd.FusedAdam).
 *
 * A header and a symbol prefix of its own (gcopt_): include/gcgcn.h is the core ABI, whose recorded symbol table
 * (tests/golden/abi_signatures.json) this extension leaves exactly as it is; its own table is recorded in
 * tests/golden/abi_signatures_optim.json and held by tests/test_optim_decay_cpu.py the same way (declared == recorded ==
 * exported).  gcgcn_amd/_lib.py binds both headers.  The calls follow the core's conventions: int status (0 = ok, message from
 * gcgcn_last_error), every device pointer as void*, the stream last.  gcgcn_adam_step / gcgcn_adam_step_dev (gcgcn.h) are what
 * this is an extension OF: plain Adam goes on through them. */
#ifndef GCGCN_OPTIM_H
#define GCGCN_OPTIM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ONE table spans every parameter group of the step.  table (device memory): n_tensors records of 72 bytes, sorted by
 * block_begin (a tensor owns ceil(numel / 1024) consecutive workgroups starting there),
 *   { float* p; const float* g; float* m; float* v; float* vmax; int64 numel; int64 block_begin;
 *     float step_size; float inv_bc2_sqrt;        -- gcopt_adamw_step_dev: these 8 bytes are `float* step`, the tensor's counter
 *     int32 group; int32 pad; }
 * vmax is amsgrad's max_exp_avg_sq (NULL in a group without amsgrad); group indexes `groups` (device memory): n_groups
 * records of 48 bytes
 *   { double beta1; double beta2; double eps; double weight_decay;
 *     double lr;                                  -- gcopt_adamw_step_dev: these 8 bytes are `const float* lr`, a device scalar
 *     uint32 flags; uint32 pad; }
 * flags: 1 weight_decay is L2, 2 weight_decay is decoupled (at most one of the two; neither: no decay), 4 amsgrad, 8 maximize,
 * 16 no bias correction (step_size = lr, inv_bc2_sqrt = 1; the host form takes both from the row either way).
 * Per element, fp32, torch.optim.Adam's single-tensor path: g <- -g (maximize); g <- g * coef (_dev, rounded on its own);
 * g <- g + wd p (L2); p <- p * (1 - lr wd) (decoupled, the factor rounded from double); the moments as gcgcn_adam_step;
 * vmax <- max(vmax, v) and the denominator from vmax (amsgrad).
 * gcopt_adamw_step: one launch; step_size = lr / (1 - beta1^t), inv_bc2_sqrt = 1 / sqrt(1 - beta2^t) decided by the host.
 * gcopt_adamw_step_dev: gcgcn_adam_step_dev's three stages over the whole table -- ONE norm, ONE coef = min(1, max_norm /
 * (norm + 1e-6)) and ONE *grad_norm for all groups (max_norm > 0 only; grad_norm may be NULL); every tensor's counter advanced
 * and its factors computed in double from ITS group's lr -- three launches with max_norm > 0, two without, whatever n_groups
 * is; a non-finite norm propagates into the parameters; no float atomics, no host read, allocation or synchronisation.
 * Every one of the n_groups records is read (gcopt_adamw_step_dev follows each record's lr), whether a row refers to it or not:
 * hand over records of groups that have rows only (gcgcn_amd/optim.py: pack_adamw_image).
 * ws: device memory, 16-byte aligned, ws_bytes >= gcopt_adamw_ws_bytes(n_tensors, n_groups, total_blocks) (-1: bad arguments). */
int64_t gcopt_adamw_ws_bytes(int n_tensors, int n_groups, int64_t total_blocks);
int gcopt_adamw_step(int n_tensors, const void* table, int n_groups, const void* groups, int64_t total_blocks, void* stream);
int gcopt_adamw_step_dev(int n_tensors, const void* table, int n_groups, const void* groups, int64_t total_blocks, double max_norm,
                         void* ws, int64_t ws_bytes, float* grad_norm, void* stream);

#ifdef __cplusplus
}
#endif
#endif
