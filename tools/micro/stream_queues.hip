// Which way of creating the engine's four chain streams (main, encoder side, AR, vocoder) gives each a hardware queue of its own, whatever
// the size of the runtime's queue pool?  Stand-alone (HIP runtime only); one mode per process, because streams that stay alive keep their
// pool entries:
//     stream_queues plain | mask | prio [n_host_streams = 3]
// The process first uses the null stream and n_host_streams plain non-blocking streams (a host application's own -- PyTorch's), then
// creates four more streams the given way and reports, for every pair of them, whether the two run concurrently (csrc/stream_overlap.h).
//   plain  hipStreamCreateWithFlags(hipStreamNonBlocking): entries of the shared pool
//   mask   hipExtStreamCreateWithCUMask with all CUs enabled: a queue outside the pool
//   prio   hipStreamCreateWithPriority(hipStreamNonBlocking): AR and vocoder at the highest priority, the other two at normal -- one pool per level
// build: hipcc --offload-arch=gfx950 -O2 -I streamvoiceanon_amd/csrc tools/micro/stream_queues.hip -o tools/micro/stream_queues
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "stream_overlap.h"
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("err %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "plain";
    const int n_host = argc > 2 ? atoi(argv[2]) : 3;
    if (n_host < 0 || n_host > 8) { printf("n_host_streams in 0 .. 8\n"); return 1; }
    int* d_words = nullptr;
    CK(hipMalloc((void**)&d_words, 2 * sizeof(int)));
    // the host application's streams, used once so that each holds its queue
    hipStream_t host[8];
    hipLaunchKernelGGL(sva_overlap::setter_kernel, dim3(1), dim3(1), 0, 0, d_words);
    for (int i = 0; i < n_host; ++i) {
        CK(hipStreamCreateWithFlags(&host[i], hipStreamNonBlocking));
        hipLaunchKernelGGL(sva_overlap::setter_kernel, dim3(1), dim3(1), 0, host[i], d_words);
    }
    CK(hipDeviceSynchronize());
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    int prio_least = 0, prio_greatest = 0;
    CK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    const char* names[4] = {"main", "aux0", "sa", "sv"};
    hipStream_t st[4];
    for (int i = 0; i < 4; ++i) {
        if (!strcmp(mode, "mask")) {
            uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int c = 0; c < prop.multiProcessorCount && c < 256; ++c) mask[c >> 5] |= 1u << (c & 31);
            CK(hipExtStreamCreateWithCUMask(&st[i], 8, mask));
        } else if (!strcmp(mode, "prio")) {
            CK(hipStreamCreateWithPriority(&st[i], hipStreamNonBlocking, i >= 2 ? prio_greatest : 0));
        } else {
            CK(hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking));
        }
        hipLaunchKernelGGL(sva_overlap::setter_kernel, dim3(1), dim3(1), 0, st[i], d_words);
    }
    CK(hipDeviceSynchronize());
    const char* env = getenv("GPU_MAX_HW_QUEUES");
    printf("mode %s, %d host streams + the null stream first, %d CUs, priority range %d (least) .. %d (greatest), GPU_MAX_HW_QUEUES=%s\n", mode, n_host,
           prop.multiProcessorCount, prio_least, prio_greatest, env ? env : "(unset)");
    for (int i = 0; i < 4; ++i) {
        unsigned flags = 0;
        int prio = 0;
        CK(hipStreamGetFlags(st[i], &flags));
        CK(hipStreamGetPriority(st[i], &prio));
        printf("  %-4s flags 0x%x (%s) priority %d\n", names[i], flags, (flags & hipStreamNonBlocking) ? "non-blocking" : "BLOCKS against the null stream", prio);
    }
    int ok[6];
    CK(sva_overlap::pairs_of_four(st, d_words, ok));
    int k = 0, all = 1;
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j, ++k) {
            printf("  %-4s | %-4s : %s\n", names[i], names[j], ok[k] ? "concurrent" : "SERIALISED (waiter timed out)");
            all &= ok[k];
        }
    // each of the four against the host application's streams (informational: sharing with an idle stream costs nothing)
    for (int i = 0; i < 4; ++i)
        for (int j = -1; j < n_host; ++j) {
            int c = 0;
            CK(sva_overlap::pair_concurrent(st[i], j < 0 ? (hipStream_t)0 : host[j], d_words, &c));
            if (!c) printf("  %-4s shares a queue with (or blocks against) %s\n", names[i], j < 0 ? "the null stream" : "a host stream");
        }
    printf("mode %s: %s\n", mode, all ? "all six pairs concurrent" : "NOT all pairs concurrent");
    return 0;
}
