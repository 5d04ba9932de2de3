// api.hip -- version, status strings and the per-device CU-count cache of libasd_hip.so.
#include "common.hpp"

#include <atomic>

namespace asd {

namespace {
constexpr int kMaxDevices = 64;
std::atomic<int> g_cus[kMaxDevices];  // 0 = not queried yet
}  // namespace

int current_device_cus() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    const int n = asd_device_cu_count(dev);
    return n > 0 ? n : 256;
}

}  // namespace asd

ASD_EXPORT int asd_version(void) {
    return ASD_VERSION_MAJOR * 10000 + ASD_VERSION_MINOR * 100 + ASD_VERSION_PATCH;
}

ASD_EXPORT const char* asd_status_string(int status) {
    switch (status) {
        case ASD_OK: return "ok";
        case ASD_ERR_INVALID_ARG: return "invalid argument";
        case ASD_ERR_UNSUPPORTED: return "unsupported size or dtype";
        case ASD_ERR_WORKSPACE: return "workspace too small or misaligned";
        case ASD_ERR_HIP: return "HIP runtime error";
        case ASD_ERR_ALIGNMENT: return "misaligned operand";
        default: return "unknown status";
    }
}

ASD_EXPORT size_t asd_sampling_rows_bytes(int B) {
    return B > 0 ? static_cast<size_t>(B) * ASD_SAMPLING_ROW_BYTES : 0;
}

// host only: every field comes from the function the scalar launchers form it with (common.hpp)
ASD_EXPORT int asd_sampling_rows_pack(const float* inv_temperature, const int32_t* top_k, const float* top_p, const float* min_p,
                                      int B, int V, int dtype, void* packed) {
    using namespace asd;
    if (B < 0 || V < 1) return ASD_ERR_INVALID_ARG;
    if (dtype_size(dtype) == 0) return ASD_ERR_UNSUPPORTED;
    if (B == 0) return ASD_OK;
    if (!inv_temperature || !packed) return ASD_ERR_INVALID_ARG;
    for (int b = 0; b < B; ++b) {
        if (!valid_inv_temperature(inv_temperature[b])) return ASD_ERR_INVALID_ARG;
        if (top_p && top_p[b] != top_p[b]) return ASD_ERR_INVALID_ARG;
        if (min_p && !valid_min_p(min_p[b])) return ASD_ERR_INVALID_ARG;
    }
    SamplingRow* out = static_cast<SamplingRow*>(packed);
    for (int b = 0; b < B; ++b) {
        const float tp = top_p ? top_p[b] : 1.0f;
        const float mp = min_p ? min_p[b] : 0.0f;
        const Truncation tr = truncation(top_k ? top_k[b] : 0, tp, V, dtype);
        SamplingRow row{};
        row.c2 = log2_scale(inv_temperature[b]);
        row.top_p = tp;
        row.levels = tr.levels;
        row.top_k = tr.top_k;
        row.mp_delta = mp > 0.0f ? min_p_delta(mp, inv_temperature[b]) : -INFINITY;
        row.clamp = mp > 0.0f ? 1u : 0u;
        out[b] = row;
    }
    return ASD_OK;
}

ASD_EXPORT int asd_device_cu_count(int device) {
    if (device < 0) return ASD_ERR_INVALID_ARG;
    if (device < asd::kMaxDevices) {
        const int c = asd::g_cus[device].load(std::memory_order_relaxed);
        if (c > 0) return c;
    }
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || v <= 0)
        return ASD_ERR_HIP;
    if (device < asd::kMaxDevices) asd::g_cus[device].store(v, std::memory_order_relaxed);
    return v;
}
