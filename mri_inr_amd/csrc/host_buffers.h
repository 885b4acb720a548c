// What a caller's host buffer is to a synchronous entry point, and the one protocol every such entry point wraps around its buffers
// (SyncHostCall: msiren.hip, scores.hip, sample_grid.hip and resample.hip use it).
#pragma once
#include <cstring>

#include "host_ctx.h"

namespace mh {

// ---- the caller's host buffers -------------------------------------------------------------------------------------------
// A host range handed to a synchronous entry point is one of three things, decided per call from what the HIP runtime says about it
// (nothing is cached, nothing of the caller's is ever registered or unregistered by this library -- round 5's per-call hipHostRegister
// of pageable buffers is gone: profiles/r6/01_*):
//   HOST_PINNED    the WHOLE range lies inside ONE page-locked allocation (msiren_host_alloc, hipHostMalloc, a caller's hipHostRegister,
//                  a pinned torch tensor): kernels and DMA copies work on it in place through `dev`;
//   HOST_PAGEABLE  no byte of it is page-locked as far as its two ends tell: copied by the runtime (hipMemcpyAsync on the pointer);
//   HOST_PARTIAL   it begins or ends inside a page-locked allocation that does not contain all of it (a caller's own partial
//                  hipHostRegister; two registrations with pageable bytes between them): the runtime refuses a copy whose range leaves
//                  the registration it starts in ("invalid argument": tools/soak.py found it in round 5) and a kernel would fault on the
//                  pageable part, so the call goes through a page-locked bounce buffer of its own -- rare, slow, correct.
enum HostKind { HOST_PAGEABLE = 0, HOST_PINNED = 1, HOST_PARTIAL = 2 };

void* host_pinned_dev(const void* p);  // device address of page-locked host memory; nullptr for ordinary pageable memory
HostKind host_range_kind(const void* host, size_t bytes, void** dev);

// Page-locked memory of one call's own (the bounce buffer of a HOST_PARTIAL range)
struct HostBounce {
    void* p = nullptr;
    HostBounce() = default;
    HostBounce(const HostBounce&) = delete;
    HostBounce& operator=(const HostBounce&) = delete;
    ~HostBounce() { if (p) (void)hipHostFree(p); }
    void* alloc(size_t n) {
        if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
        }
        return p;
    }
};

// How a synchronous call uses one of its caller's buffers.
enum HostPolicy : unsigned {
    // Always through device memory: staging, or the device buffer the call names.  Every input but the tiles of the sampling calls and of
    // a one-chunk msiren_forward_tiles.  msiren_reconstruct_slices copies its image ON PURPOSE (DMA from page-locked memory, through the
    // runtime from pageable memory): read in place every pixel would cross the link four times (32 x 32 tiles at a stride of 16;
    // profiles/r5/09_*).  Modulations are read once per unit of the trunk: copied as well.
    HOST_COPY = 0,
    // The kernels read / write the range in place where it is page-locked (the device view of the caller's allocation; of the bounce
    // buffer where the range is page-locked in part); a pageable range is copied.
    HOST_IN_PLACE = 1,
    // Staged, but the call enqueues the copies itself through host_src / host_dst: the chunk loops of msiren_forward_tiles and
    // msiren_encode_modulate_tiles, whose copies go chunk by chunk on alternating streams.
    HOST_OWN_COPIES = 2,
    // Staged right behind the previous buffer, without alignment padding: the second image of msiren_score_images, whose kernels ask
    // for 4-byte alignment only and whose two images have always shared one staging buffer of exactly their size.
    HOST_PACKED = 4,
};

// One synchronous call on host pointers:
//     SyncHostCall io(h, stream);
//     const int a = io.in(...), b = io.out(...);   classify each buffer (once), bounce what is page-locked in part; nothing is enqueued
//     if ((rc = io.begin())) return rc;             staging on the handle (grow-only, every size known: nothing is reallocated while the
//                                                   call's work is queued), then the H2D copies in the order of in()
//     ... the *_dev work on io.src<T>(a) / io.dst<T>(b) ...
//     return io.finish();                           D2H of what was not in place, the wait, bounce buffers back to the caller
// From begin() until a finish() that succeeded the destructor waits for the handle's streams -- a call that leaves early (a failed launch,
// a failed copy) may have copies in flight on the caller's buffers or on a bounce buffer -- and the bounce buffers are members, so they
// are freed behind that wait whatever the caller declares in which order.  A bounce buffer reaches the caller behind a successful wait only.
//
// What is used in place (everything else: copied / staged):
//     forward_mods, forward_latent, encode_tiles, modulate, score_images   --
//     memcpy_h2d / memcpy_d2h                                              -- (the device side is the caller's)
//     forward_tiles, ONE chunk                  tiles; out; host-side domain check
//     reconstruct_slices(_scaled)               recon
//     reconstruct_slices_grad                   recon (optional), grad
//     sample_{mods,tiles}                       tiles; out; host-side domain check
//     sample_grad_{mods,tiles}                  tiles; out (optional), grad
//     sample_ragged_(grad_)mods                 out (optional) / grad
//     resample_slices(_grad)                    out (optional) / grad
class SyncHostCall {
public:
    static constexpr int kMax = 7;  // buffers per direction (msiren_align_volume_solve_group_r stages seven inputs)
    // wait_all: finish() waits for all the handle's streams (sync_all) instead of `stream` alone
    SyncHostCall(msiren_ctx* h, int stream, bool wait_all = false) : h_(h), stream_(stream), wait_all_(wait_all) {}
    SyncHostCall(const SyncHostCall&) = delete;
    SyncHostCall& operator=(const SyncHostCall&) = delete;
    ~SyncHostCall();

    // -> the buffer's number for src / dst.  `dev`: the device memory the work reads the input from / leaves the output in (per-stream
    // scratch such as sc.coords, sc.mods, sc.latent; ensured by the caller); null: staging.  A null `host` (an optional output left
    // out): dst() is null, nothing is copied.
    int in(const void* host, size_t bytes, unsigned policy, void* dev = nullptr) { return add(in_, nin_, in_bytes_, (void*)host, bytes, policy, dev, true); }
    int out(void* host, size_t bytes, unsigned policy, const void* dev = nullptr) { return add(out_, nout_, out_bytes_, host, bytes, policy, (void*)dev, false); }
    int begin();
    template <typename T> const T* src(int i) const { return (const T*)device(in_[i], h_->stage_in); }
    template <typename T> T* dst(int i) const { return (T*)device(out_[i], h_->stage_out); }
    // the host side of a HOST_OWN_COPIES buffer: the caller's pointer, or the bounce buffer of a range that is page-locked in part
    template <typename T> const T* host_src(int i) const { return (const T*)in_[i].p; }
    template <typename T> T* host_dst(int i) const { return (T*)out_[i].p; }
    int finish();  // may be called again behind further work on the stream (recheck does)
    // The host-side domain check of a call whose trunk was launched with mode.host_check (host_ctx.h: HostCheck), behind finish(): where
    // the trunk met a modulation outside the fp16 domain, the batch once more on the exact-fp32 trunk at the call's coordinates (the
    // conditional kernel, its condition pointed at the word that has just been read), then finish() once more.
    int recheck(const HostCheck& hc, const CoordSet& cs);

private:
    struct Item {
        void* host = nullptr;  // the caller's pointer
        void* p = nullptr;     // what copies use: `host`, or the bounce buffer
        void* dev = nullptr;   // the device side: the page-locked view in place, or the buffer the call named; null: staging at `off`
        size_t n = 0, off = 0;
        bool copy = false;     // begin() / finish() copy it
        HostBounce b;
    };
    int add(Item* items, int& count, size_t& staged, void* host, size_t n, unsigned policy, void* dev, bool input);
    static void* device(const Item& it, const DevBuf& stage) { return !it.host ? nullptr : it.dev ? it.dev : (char*)stage.p + it.off; }

    msiren_ctx* h_;
    int stream_;
    bool wait_all_, ok_ = true, too_many_ = false, armed_ = false;
    int nin_ = 0, nout_ = 0;
    size_t in_bytes_ = 0, out_bytes_ = 0;  // of staging, every buffer at a multiple of 128 (HOST_PACKED: none)
    Item in_[kMax], out_[kMax];
};

}  // namespace mh
