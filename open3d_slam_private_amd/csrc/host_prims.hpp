// host_prims.hpp -- host primitives the entry points share: rocPRIM's temporary-storage protocol, scans and sorts on it,
// the total of a flag array, the sort of voxel keys into runs (sort_runs), the crop configuration, staged inputs; the outputs of the operators that have a host and a
// device-pointer form (StagedOut: one declaration per output gives its device pointer, its share of the staging buffer and
// its copy-back; copy_out for an output held in a working buffer); the pack / bounding box / non-finite front of the box
// filters
// Part of the single translation unit reg_core.hip (included there after host_handle.hpp, which completes reg_handle and
// HIPCHK, and before host_target.hpp; not a standalone header).
#pragma once

#define REGCHK(call)                                                                           \
    do {                                                                                       \
        const reg_status s_ = (call);                                                          \
        if (s_ != REG_OK) return s_;                                                           \
    } while (0)

// rocPRIM's two-phase protocol.  call(tmp, bytes) is ONE spelling of the rocPRIM call: with tmp == nullptr it reports the
// bytes it needs, with storage it runs.  tmp_reserve is the first phase alone, for a call that runs later on the same
// arguments; with_tmp is both.  The working call never sees a null pointer (to rocPRIM that is another size query: nothing
// would run and no error would be raised), whatever size was reported.
template <class F>   // F: hipError_t(void* tmp, size_t& bytes)
static reg_status tmp_reserve(reg_handle* h, DevBuf& tmp, size_t& bytes, F call) {
    bytes = 0;
    HIPCHK(h, call((void*)nullptr, bytes));
    HIPCHK(h, tmp.reserve(bytes ? bytes : 1));
    return REG_OK;
}
template <class F>
static reg_status with_tmp(reg_handle* h, DevBuf& tmp, F call) {
    size_t bytes = 0;
    REGCHK(tmp_reserve(h, tmp, bytes, call));
    HIPCHK(h, call(tmp.p, bytes));
    return REG_OK;
}

// out[i] = in[0] + ... + in[i - 1] (exclusive) / ... + in[i] (inclusive); in == out is allowed
static reg_status scan_excl(reg_handle* h, DevBuf& tmp, const uint32_t* in, uint32_t* out, size_t n) {
    return with_tmp(h, tmp, [&](void* t, size_t& b) {
        return rocprim::exclusive_scan(t, b, in, out, 0u, n, rocprim::plus<uint32_t>(), h->stream);
    });
}
static reg_status scan_incl(reg_handle* h, DevBuf& tmp, const uint32_t* in, uint32_t* out, size_t n) {
    return with_tmp(h, tmp, [&](void* t, size_t& b) {
        return rocprim::inclusive_scan(t, b, in, out, n, rocprim::plus<uint32_t>(), h->stream);
    });
}

// Stable ascending radix sorts on the key bits [begin_bit, end_bit)
template <class K, class V, class Size>
static reg_status sort_pairs(reg_handle* h, DevBuf& tmp, K* keys, K* keys_out, V* vals, V* vals_out, Size n, int begin_bit,
                             int end_bit) {
    return with_tmp(h, tmp, [&](void* t, size_t& b) {
        return rocprim::radix_sort_pairs(t, b, keys, keys_out, vals, vals_out, n, begin_bit, end_bit, h->stream);
    });
}
template <class K, class Size>
static reg_status sort_keys(reg_handle* h, DevBuf& tmp, K* keys, K* keys_out, Size n, int begin_bit, int end_bit) {
    return with_tmp(h, tmp, [&](void* t, size_t& b) {
        return rocprim::radix_sort_keys(t, b, keys, keys_out, n, begin_bit, end_bit, h->stream);
    });
}

// Total of n 0 / 1 flags from their exclusive scan: enqueues the read-backs of the last offset and the last flag into
// tail[2] (n == 0: nothing).  The caller synchronises -- usually with further words in flight -- and then reads flag_total.
static reg_status flag_total_async(reg_handle* h, const uint32_t* flags, const uint32_t* offs, int64_t n, uint32_t tail[2]) {
    tail[0] = tail[1] = 0;
    if (n <= 0) return REG_OK;
    HIPCHK(h, hipMemcpyAsync(&tail[0], offs + (n - 1), 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&tail[1], flags + (n - 1), 4, hipMemcpyDeviceToHost, h->stream));
    return REG_OK;
}
static inline int64_t flag_total(const uint32_t tail[2]) { return (int64_t)tail[0] + (int64_t)tail[1]; }
// The whole of it where no further word is read back in the same synchronisation: scan, read-back, one synchronisation
static reg_status scan_total(reg_handle* h, const uint32_t* flags, uint32_t* offs, int64_t n, int64_t* total) {
    uint32_t tail[2];
    REGCHK(scan_excl(h, h->rp_tmp, flags, offs, (size_t)n));
    REGCHK(flag_total_async(h, flags, offs, n, tail));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *total = flag_total(tail);
    return REG_OK;
}

// "Sort the keys, find the runs" of n > 0 voxel keys: the stable sort of (keys, vals) on the 3 * kVoxBits key bits into
// (sorted, svals), heads = 1 at the first position of every run of equal sorted keys, run = the exclusive scan of heads.
// Enqueues the read-back of the number of runs into tail and does not synchronise: the caller does, then reads flag_total.
static reg_status sort_runs(reg_handle* h, const RunArrays& a, int64_t n, uint32_t tail[2]) {
    REGCHK(sort_pairs(h, h->rp_tmp, a.keys, a.sorted, a.vals, a.svals, (size_t)n, 0, 3 * kVoxBits));
    k_vox_heads<<<grid_for(n), 256, 0, h->stream>>>(a.sorted, n, a.heads);
    REGCHK(scan_excl(h, h->rp_tmp, a.heads, a.run, (size_t)n));
    return flag_total_async(h, a.heads, a.run, n, tail);
}

// reg_crop (null: no cropping) -> the kernels' CropCfg; false: unknown type
static bool crop_cfg(const reg_crop* crop, CropCfg* c) {
    std::memset(c, 0, sizeof(*c));
    if (!crop) return true;
    if (crop->type < REG_CROP_NONE || crop->type > REG_CROP_CYLINDER) return false;
    c->type = crop->type;
    c->cx = crop->center[0];
    c->cy = crop->center[1];
    c->cz = crop->center[2];
    c->rmin = crop->radius_min;
    c->rmax = crop->radius_max;
    c->zmin = crop->min_z;
    c->zmax = crop->max_z;
    return true;
}

// Uploads (host input) or reads in place (device input, or none) `count` elements; *out is the device pointer.
template <class T>
static hipError_t staged_input(reg_handle* h, DevBuf& buf, const T* src, size_t count, int on_device, const T** out) {
    *out = src;
    if (!src || on_device) return hipSuccess;
    const hipError_t e = buf.reserve(count * sizeof(T));
    if (e != hipSuccess) return e;
    *out = buf.as<T>();
    return hipMemcpyAsync(buf.p, src, count * sizeof(T), hipMemcpyHostToDevice, h->stream);
}

// The outputs of an operator that has a host and a device-pointer form.  The entry point declares each output once --
// add(the caller's pointer or null, elements per row) -- calls reserve(row capacity), hands at<T>(slot) to its kernels and
// ends with copy_back(rows).  Device-pointer form: at() is the caller's pointer and nothing is copied.  Host form: at() is a
// 16-byte aligned slice of `buf`, and copy_back enqueues rows * bytes-per-row of every output the caller asked for on
// h->stream (rows == 0: nothing); the caller synchronises.  An absent output is null, unless it was declared `always`
// (the kernel writes it whether the caller wants it or not): then it is a scratch slice in both forms.  at() reads buf.p
// when it is called, so reserve() comes first.
struct StagedOut {
    struct Slot {
        void* user;
        size_t row_bytes, off;
        bool staged;
    };
    reg_handle* h;
    DevBuf& buf;
    const int on_device;
    Slot s[REG_MAX_FIELDS + 8];   // the widest caller: xyz, idx and REG_MAX_FIELDS descriptor fields
    int n = 0;
    StagedOut(reg_handle* h_, DevBuf& buf_, int on_device_) : h(h_), buf(buf_), on_device(on_device_) {}
    template <class T>
    int add(T* user, size_t per_row, bool always = false) {
        s[n] = {user, per_row * sizeof(T), 0, on_device ? (always && !user) : (always || user)};
        return n++;
    }
    hipError_t reserve(size_t rows) {
        size_t bytes = 0;
        for (int i = 0; i < n; ++i)
            if (s[i].staged) {
                s[i].off = bytes;
                bytes += (std::max<size_t>(rows, 1) * s[i].row_bytes + 15) & ~(size_t)15;
            }
        return buf.reserve(bytes);
    }
    template <class T>
    T* at(int i) const {
        return s[i].staged ? (T*)((char*)buf.p + s[i].off) : (T*)(on_device ? s[i].user : nullptr);
    }
    hipError_t copy_back(int i, size_t rows) const {   // one output, for an operator whose outputs differ in their rows
        if (on_device || !s[i].user || rows == 0) return hipSuccess;
        return hipMemcpyAsync(s[i].user, at<char>(i), rows * s[i].row_bytes, hipMemcpyDeviceToHost, h->stream);
    }
    hipError_t copy_back(size_t rows) const {
        for (int i = 0; i < n; ++i) {
            const hipError_t e = copy_back(i, rows);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
};

// An output that already lives in a working buffer: `bytes` from there to the caller's array (null: not wanted; the buffer
// itself, where a kernel wrote through the caller's device pointer: nothing to do), enqueued on h->stream.
static hipError_t copy_out(reg_handle* h, void* user, const void* src, size_t bytes, int on_device) {
    if (!user || user == src || bytes == 0) return hipSuccess;
    return hipMemcpyAsync(user, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream);
}

// The common front of the box-based filters: packs the cloud into px (n x 3), takes its bounding box and rejects
// non-finite input ("<who>: non-finite input").  misc (h->f_misc, >= 10 words) is left as [0..2] min, [3..5] max
// (orderable keys), [6] the non-finite flag, [7..9] zero; box receives words 0..6.  One synchronisation.
static reg_status pack_cloud_box(reg_handle* h, const char* who, const float* d_in, int64_t xyz_stride, int N, float* px,
                                 uint32_t box[7]) {
    const uint32_t misc0[10] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    HIPCHK(h, hipMemcpyAsync(h->f_misc.p, misc0, sizeof(misc0), hipMemcpyHostToDevice, h->stream));
    k_ssn_pack<<<grid_for(N), 256, 0, h->stream>>>(d_in, xyz_stride, N, px, h->f_misc.as<uint32_t>());
    HIPCHK(h, hipMemcpyAsync(box, h->f_misc.p, 7 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (box[6]) {
        h->err = std::string(who) + ": non-finite input";
        return REG_BAD_ARGUMENT;
    }
    return REG_OK;
}
