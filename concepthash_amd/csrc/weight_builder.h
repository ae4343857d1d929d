// Weight ingestion shared by the handles that are built from named fp32 tensors (ch_model_create: model.hip, ch_text_create:
// text_model.hip): look a tensor up by its state_dict key, check its size, copy or convert it to the device, into memory of the
// handle's owner (device_owner.h).  ch_tensor.data may be a host or a device pointer (hipMemcpyDefault).
#pragma once
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/concepthash_hip.h"
#include "ch_common.h"
#include "device_owner.h"
#include "kernels.h"

struct ChWeightBuilder {
    ChDeviceOwner &owner;                    // the handle's: every weight and workspace block comes from it
    std::map<std::string, const ch_tensor *> tab;
    std::set<std::string> used;              // names that find() has handed out (what is left over is unknown to the model)
    hipStream_t s = nullptr;
    bool ok = true;

    explicit ChWeightBuilder(ChDeviceOwner &o) : owner(o) {}
    void *alloc(size_t nbytes, bool zero = false) {
        void *p = owner.alloc(nbytes, zero);
        if (!p) ok = false;
        return p;
    }
    const ch_tensor *find(const std::string &name, int64_t numel) {
        auto it = tab.find(name);
        if (it == tab.end()) {
            ch_set_error("missing tensor '" + name + "'");
            ok = false;
            return nullptr;
        }
        if (it->second->numel != numel) {
            ch_set_error("tensor '" + name + "' has " + std::to_string(it->second->numel) + " elements, expected " +
                         std::to_string(numel));
            ok = false;
            return nullptr;
        }
        used.insert(name);
        return it->second;
    }
    bool has(const std::string &name) { return tab.count(name) != 0; }
    // fp32 -> fp32 device, into dst (a slice of a fused tensor) or a fresh allocation
    float *f32(const std::string &name, int64_t numel, float *dst = nullptr) {
        const ch_tensor *t = find(name, numel);
        if (!t) return nullptr;
        if (!dst) dst = (float *)alloc(sizeof(float) * numel);
        if (!dst) return nullptr;
        if (hipMemcpy(dst, t->data, sizeof(float) * numel, hipMemcpyDefault) != hipSuccess) {
            ch_set_error("hipMemcpy failed for '" + name + "'");
            ok = false;
        }
        return dst;
    }
    float *f32_zeros(int64_t numel) { return (float *)alloc(sizeof(float) * numel, true); }
    // fp32 [rows, cols] -> bf16 device [rows, cols_pad] written into dst (or a fresh allocation)
    bf16_t *bf16(const std::string &name, int64_t rows, int cols, int cols_pad, bf16_t *dst = nullptr) {
        const ch_tensor *t = find(name, rows * cols);
        if (!t) return nullptr;
        ChDeviceTemp tmp;
        if (tmp.get(sizeof(float) * rows * cols)) {
            ok = false;
            return nullptr;
        }
        if (!dst) dst = (bf16_t *)alloc(sizeof(bf16_t) * rows * cols_pad);
        if (dst) {
            if (hipMemcpy(tmp.as<float>(), t->data, sizeof(float) * rows * cols, hipMemcpyDefault) != hipSuccess) ok = false;
            if (ch_convert_bf16(tmp.as<float>(), rows, cols, cols_pad, dst, s) != 0) ok = false;
            if (hipStreamSynchronize(s) != hipSuccess) ok = false;
        }
        return dst;
    }
};
