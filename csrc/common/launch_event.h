// Kernel launch that can carry an event (HIP sources only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

namespace mx {
// With `done` set the event is the kernel's stop event: it completes with the kernel, so a stream
// or the host waiting for it waits for the kernel itself and no hipEventRecord (a barrier packet
// of its own behind the kernel) follows.  Null: a plain launch (graph capture, and every path that
// records its event after more than this kernel).
template <typename... Params, typename... Args>
inline void launch_with_event(hipEvent_t done, void (*kernel)(Params...), dim3 grid, dim3 block, hipStream_t stream,
                              Args... args) {
    if (done)
        hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, nullptr, done, 0, static_cast<Params>(args)...);
    else
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, static_cast<Params>(args)...);
}
}  // namespace mx
