// libmsiren.so, host side: classification of a caller's host range and the protocol of a synchronous host-pointer call (host_buffers.h).
#include "host_buffers.h"

namespace mh {

// Device address of page-locked host memory; nullptr for ordinary pageable memory.
void* host_pinned_dev(const void* p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // (pageable memory is "invalid value" to the runtime: not an error of ours)
        return nullptr;
    }
    return a.type == hipMemoryTypeHost ? a.devicePointer : nullptr;
}

HostKind host_range_kind(const void* host, size_t bytes, void** dev) {
    *dev = nullptr;
    if (!host || !bytes) return HOST_PAGEABLE;
    void* const d = host_pinned_dev(host);
    if (!d) return (bytes > 1 && host_pinned_dev((const char*)host + bytes - 1)) ? HOST_PARTIAL : HOST_PAGEABLE;
    // both ends inside page-locked memory is not enough (two allocations, pageable bytes in between; on this platform the device
    // address of page-locked memory usually EQUALS its host address, so "d_last == d + bytes - 1" proves nothing): the allocation
    // that holds the first byte must hold the last one -- its start and size from the runtime.  hipPointerGetAttribute's RANGE_START_ADDR
    // / RANGE_SIZE answer for hipHostMalloc blocks and hipHostRegister'ed ranges alike, at interior pointers too, on both runtimes a
    // process can end up on; hipMemGetAddressRange reports base 0 for registered memory (tools/ptr_range_probe.py, profiles/r6/05_*).
    void* start = nullptr;
    size_t size = 0;
    if (hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, (hipDeviceptr_t)host) != hipSuccess ||
        hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, (hipDeviceptr_t)host) != hipSuccess || !start) {
        (void)hipGetLastError();
        return HOST_PARTIAL;  // (the runtime cannot name the allocation: do not trust the range)
    }
    if ((uintptr_t)host < (uintptr_t)start || (uintptr_t)host + bytes > (uintptr_t)start + size) return HOST_PARTIAL;
    *dev = d;
    return HOST_PINNED;
}

int SyncHostCall::add(Item* items, int& count, size_t& staged, void* host, size_t n, unsigned policy, void* dev, bool input) {
    if (count == kMax) {  // (begin() refuses the call)
        too_many_ = true;
        return 0;
    }
    Item& it = items[count];
    if (!host || !n) return count++;
    it.host = it.p = host;
    it.n = n;
    void* view = nullptr;
    if (host_range_kind(host, n, &view) == HOST_PARTIAL) {
        if (it.b.alloc(n)) {
            it.p = it.b.p;
            if (input) std::memcpy(it.p, host, n);
            if (policy & HOST_IN_PLACE) view = host_pinned_dev(it.p);
        } else ok_ = false;
    }
    if ((policy & HOST_IN_PLACE) && view) {
        it.dev = view;
    } else {
        it.copy = !(policy & HOST_OWN_COPIES);
        it.dev = dev;
        if (!dev) {
            // 128: less than 127 * 1.25 bytes of padding against the 256 bytes of slack that ensure() gave each of the separate buffers
            // an arena replaces, so the arena is never the larger; HOST_PACKED: no padding, where one buffer held both before
            it.off = (policy & HOST_PACKED) ? staged : (staged + 127) & ~(size_t)127;
            staged = it.off + n;
        }
    }
    return count++;
}

int SyncHostCall::begin() {
    if (too_many_) return fail(MSIREN_E_INVALID, "more than %d host buffers per direction in one call", kMax);
    if (!ok_) return fail(MSIREN_E_HIP, "no page-locked memory for a bounce buffer");
    int rc;
    if ((rc = ensure(h_, h_->stage_in, in_bytes_)) || (rc = ensure(h_, h_->stage_out, out_bytes_))) return rc;
    armed_ = true;
    for (int i = 0; i < nin_; ++i)
        if (in_[i].copy) HIPCHK(hipMemcpyAsync(device(in_[i], h_->stage_in), in_[i].p, in_[i].n, hipMemcpyHostToDevice, h_->sc[stream_].s));
    return 0;
}

int SyncHostCall::finish() {
    for (int i = 0; i < nout_; ++i)
        if (out_[i].copy) HIPCHK(hipMemcpyAsync(out_[i].p, device(out_[i], h_->stage_out), out_[i].n, hipMemcpyDeviceToHost, h_->sc[stream_].s));
    if (wait_all_) {
        const int rc = sync_all(h_);
        if (rc) return rc;
    } else {
        HIPCHK(hipStreamSynchronize(h_->sc[stream_].s));
    }
    armed_ = false;
    for (int i = 0; i < nout_; ++i)
        if (out_[i].b.p) std::memcpy(out_[i].host, out_[i].b.p, out_[i].n);
    return 0;
}

int SyncHostCall::recheck(const HostCheck& hc, const CoordSet& cs) {
    if (!hc.armed || (unsigned)h_->status_host[8] != hc.epoch) return 0;
    Call fix = with_coords(make_call(h_, true), cs);
    fix.stream = stream_;
    armed_ = true;
    const int rc = launch_trunk_f32_cond(h_, fix, hc.mods, hc.B, hc.out, h_->status_dev + 8, hc.epoch);
    return rc ? rc : finish();
}

SyncHostCall::~SyncHostCall() {
    if (!armed_) return;
    for (auto& c : h_->sc)
        if (c.s) (void)hipStreamSynchronize(c.s);
}

}  // namespace mh
