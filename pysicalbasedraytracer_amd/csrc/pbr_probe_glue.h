// pbr_probe_glue.h — what a probe compiled in a translation unit of its own (pbr_bsdf_probe.hip) needs
// of a context: the uploaded scene's device view, its lobe kinds, and a round trip through the
// context's scratch buffers on its stream.  Defined in pbr_kernels.hip, which owns pbr_hip_ctx.  The
// probes' kernels are kept out of pbr_kernels.hip so that its device code stays what it was.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>

#include "../../include/pbr_hip.h"
#include "pbr_layout.h"

namespace pbr {

// launch(the scene's device view — zeros without a scene —, the context's stream, the input on the
// device, the output on the device)
using ProbeLaunch = std::function<void(const DeviceScene& S, hipStream_t stream, const void* in, void* out)>;

int probe_fail(pbr_hip_ctx* ctx, int code, const char* msg);   // records msg as the context's error; returns code
// scene_lobe_kinds and the number of lobe templates (2 per material); PBR_E_NOSCENE without a scene
int probe_scene_info(pbr_hip_ctx* ctx, int* lobeKinds, int* nTemplates);
// n > 0: inBytes of `in` to the device, launch, outBytes back to `out`, the stream waited for
int probe_round_trip(pbr_hip_ctx* ctx, int n, const void* in, size_t inBytes, void* out, size_t outBytes, const ProbeLaunch& launch);

}  // namespace pbr
