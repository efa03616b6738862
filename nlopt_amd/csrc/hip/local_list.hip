/* local_list.hip — the waiting list of a coroutine step, built on the device.
 *
 * A batch of local searches whose objective is a user's kernel runs as coroutines (include/nlopt_amd.h "External evaluation"): after
 * every launch of the search kernel the searches in state 1 wait for an evaluation, and one launch of the user's kernel serves them
 * all through a list of their indices (nla_userobj_evalgrad_list).  lbfgs_driver.c builds that list on the host — the records come
 * down, the list goes up, every step.  This kernel builds the same list where the records are; the host reads back one int32.
 *
 * Order: ascending search index, as the host loop's — a stream compaction, not a queue: ONE workgroup of 256 threads walks the
 * records in chunks of 256.  Per chunk each wavefront takes a ballot of "waits" and a lane's slot is the popcount of the ballot
 * below it; the four wavefront totals meet in LDS; the entries written so far are a running base, the same in every lane, kept in a
 * scalar register.  No atomics, nothing depends on scheduling: the list is the host's entry for entry.  At 65536 searches that is
 * 256 trips of one load, one ballot and two barriers. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/nlopt_amd.h"

__global__ __launch_bounds__(256) void local_waiting_list_kernel(const nla_local_req *__restrict__ req, int count, int32_t *__restrict__ list,
                                                                 int32_t *__restrict__ n_waiting)
{
    __shared__ int wave_total[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int base = 0;
    /* the record of the NEXT chunk is fetched before this chunk's barriers: its latency hides behind them (a trip is otherwise one
     * dependent global load long) */
    nla_local_req cur = { 0, 0 };
    if (t < count) cur = req[t];
    for (int c0 = 0; c0 < count; c0 += 256) {
        const int i = c0 + t;
        nla_local_req nxt = { 0, 0 };
        if (i + 256 < count) nxt = req[i + 256];
        const bool waits = i < count && cur.state == 1, grad = (cur.want_grad & 1) != 0;
        const unsigned long long mask = __ballot(waits);
        const int below = __popcll(mask & ((1ULL << lane) - 1ULL));
        if (lane == 0) wave_total[wave] = __popcll(mask);
        __syncthreads();
        const int t0 = wave_total[0], t1 = wave_total[1], t2 = wave_total[2], t3 = wave_total[3];
        const int before = wave == 0 ? 0 : wave == 1 ? t0 : wave == 2 ? t0 + t1 : t0 + t1 + t2;
        if (waits) list[base + before + below] = grad ? i : -(i + 1);
        base = __builtin_amdgcn_readfirstlane(base + t0 + t1 + t2 + t3);
        cur = nxt;
        __syncthreads();                                     /* the totals are overwritten by the next chunk */
    }
    if (t == 0) *n_waiting = base;
}

extern "C" int nla_k_local_waiting_list(const nla_local_req *req, int count, int32_t *list, int32_t *n_waiting, void *stream)
{
    /* (count <= 2^30: the kernel's indices i + 256 stay inside an int) */
    if (count < 0 || count > (1 << 30) || !n_waiting || (count > 0 && (!req || !list))) return (int) hipErrorInvalidValue;
    hipLaunchKernelGGL(local_waiting_list_kernel, dim3(1), dim3(256), 0, (hipStream_t) stream, req, count, list, n_waiting);
    return (int) hipGetLastError();
}

/* free device memory right now (what nlopt_amd_optimize_batch sizes its chunks from); 0: the runtime would not say */
extern "C" size_t nla_dev_mem_free_bytes(void)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void) hipGetLastError(); return 0; }
    return free_b;
}
