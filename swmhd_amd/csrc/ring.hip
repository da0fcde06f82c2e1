// y-slab ring for the multi-GPU engine: an RCCL communicator, a high-priority comm stream and the native
// step driver that overlaps the neighbour exchange with the interior rows.
//
// The reference is single-process: its periodic y-boundary is Oceananigans' in-memory halo copy (topology =
// (Periodic, Periodic, Flat), jacobian_formulation/SWMHD_example.jl:16; fill_halo_regions! inside update_state!).  With one
// process per GPU that copy becomes a ring of ncclSend/ncclRecv between y-neighbours.  Parents are x-fastest, so the Hy edge
// rows of a field (full padded width, corners included) are ONE contiguous run: every send reads the interior edge rows in
// place and every receive lands directly in the halo rows -- no pack/unpack kernels, one grouped RCCL launch per exchange.
//
// RCCL is bound at run time (dlopen of the path the host passes -- the copy PyTorch already loaded when the host is the
// Python harness) so that libswmhd.so itself carries no link-time dependency on it; single-GPU users never touch it.
#include "api_args.hpp"
#include "common.hpp"
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <dlfcn.h>
#include <memory>
#include <mutex>
#include <new>
#include <rccl/rccl.h>
#include <string>
#include <vector>

namespace {

struct RcclApi {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};

bool load_rccl(const char *path, RcclApi &api, std::string &err) {
    const char *candidates[] = {path, "librccl.so.1", "librccl.so"};
    for (const char *c : candidates) {
        if (!c || !*c) continue;
        api.handle = dlopen(c, RTLD_NOW | RTLD_LOCAL);
        if (api.handle) break;
        err = dlerror();
    }
    if (!api.handle) return false;
#define SW_SYM(field, name)                                                                \
    api.field = reinterpret_cast<decltype(api.field)>(dlsym(api.handle, name));           \
    if (!api.field) { err = std::string("missing symbol ") + name; return false; }
    SW_SYM(GetUniqueId, "ncclGetUniqueId")
    SW_SYM(CommInitRank, "ncclCommInitRank")
    SW_SYM(CommDestroy, "ncclCommDestroy")
    SW_SYM(GroupStart, "ncclGroupStart")
    SW_SYM(GroupEnd, "ncclGroupEnd")
    SW_SYM(Send, "ncclSend")
    SW_SYM(Recv, "ncclRecv")
    SW_SYM(GetErrorString, "ncclGetErrorString")
#undef SW_SYM
    return true;
}

// ---- loopback transport ---------------------------------------------------------------------------------------------------------
// K rings in ONE process on ONE GPU (RCCL refuses two ranks per device): the exchange of ring r copies its neighbours' edge rows
// into its own halo rows with hipMemcpyAsync on its comm stream, with the rendezvous semantics RCCL gives a grouped send/recv:
//   a receive completes only after the sender has reached the matching exchange   (wait for the peer's "rows ready" event)
//   a send completes only after the receiver has taken the rows                     (wait for the peer's "consumed" event)
// so that the real slab drivers run with north != south, every ring on its own pair of streams.  Events can only be waited
// for once they have been recorded, hence a HOST-side rendezvous as well: exchange number k of a ring blocks until its neighbours
// have enqueued theirs -- the rings must be driven from one host thread each, as RCCL ranks are driven from one process each.  A
// neighbour that does not arrive within the hub's timeout ends the exchange with SWMHD_ECOMM instead of blocking for ever.
struct LoopHub {
    static constexpr int MAXF = 8, SLOTS = 4;
    struct Post {
        unsigned long seq = 0;                 // number of exchanges this rank has posted (rows ready)
        unsigned long done = 0;                // number of exchanges whose receives this rank has enqueued (rows consumed)
        const char *send_s[SLOTS][MAXF] = {}, *send_n[SLOTS][MAXF] = {};
        size_t bytes[SLOTS] = {};
        int nf[SLOTS] = {};
        hipEvent_t ready[SLOTS] = {}, consumed[SLOTS] = {};
    };
    std::mutex mu;
    std::condition_variable cv;
    std::vector<Post> post;
    double timeout_s = 60.0;
    explicit LoopHub(int n) : post(n) {}
    ~LoopHub() {
        for (auto &p : post)
            for (int k = 0; k < SLOTS; ++k) { if (p.ready[k]) (void)hipEventDestroy(p.ready[k]); if (p.consumed[k]) (void)hipEventDestroy(p.consumed[k]); }
    }
};

}  // namespace

struct swmhd_ring {
    RcclApi api;
    ncclComm_t comm = nullptr;
    std::shared_ptr<LoopHub> hub;    // loopback transport (swmhd_ring_create_loopback); comm stays NULL then
    int nranks = 1, rank = 0, south = 0, north = 0;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_main = nullptr, ev_comm = nullptr;
    const void *pending = nullptr;   // first parent of the state whose y-exchange is in flight on comm_stream (NULL: none)
    std::string err;
    // optional timing of the interior launches (bench.py's roofline leg)
    std::vector<hipEvent_t> t0, t1;
    std::vector<int> trows;
    size_t tcap = 0;
};

namespace {

int fail(swmhd_ring *r, const char *what, ncclResult_t rc) {
    r->err = std::string(what) + ": " + (r->api.GetErrorString ? r->api.GetErrorString(rc) : "rccl error");
    return SWMHD_ECOMM;
}
int hipfail(swmhd_ring *r, const char *what, hipError_t e) {
    r->err = std::string(what) + ": " + hipGetErrorString(e);
    return -(int)e;
}

template <typename T> constexpr ncclDataType_t nccl_type();
template <> constexpr ncclDataType_t nccl_type<double>() { return ncclFloat64; }
template <> constexpr ncclDataType_t nccl_type<float>() { return ncclFloat32; }

// The Hy-row runs of one field that an exchange moves (x-fastest: each is ONE contiguous run of full padded rows): the southern and
// northern edge rows it sends, the south and north halo rows it receives.
struct EdgeRows {
    const char *send_s, *send_n;
    char *recv_s, *recv_n;
};
template <typename T> EdgeRows edge_rows(T *p, int Ny, int Hy, int64_t sy) {
    return {(const char *)(p + (size_t)Hy * sy), (const char *)(p + (size_t)Ny * sy), (char *)p, (char *)(p + (size_t)(Ny + Hy) * sy)};
}

// The exchange through the loopback hub (see LoopHub): post my edge rows, copy my neighbours' into my halos, wait until mine were taken.
// sides: bit 0 = the south neighbour, bit 1 = the north neighbour (a chain's end ranks post and take one side only; the other ranks
// count exchanges all the same, so exchange k of a rank always pairs with exchange k of its neighbours).  rows(f): field f's EdgeRows.
template <class Rows>
int loopback_exchange(swmhd_ring *r, const Rows &rows, int nf, size_t bytes, int sides, hipStream_t s) {
    LoopHub &h = *r->hub;
    hipError_t e;
    unsigned long k;
    int slot;
    {   // (1) rows ready: everything enqueued on s so far precedes the neighbours' reads
        std::unique_lock<std::mutex> lk(h.mu);
        LoopHub::Post &me = h.post[r->rank];
        k = me.seq + 1; slot = (int)(k % LoopHub::SLOTS);
        if (!me.ready[slot] && (e = hipEventCreateWithFlags(&me.ready[slot], hipEventDisableTiming)) != hipSuccess) return hipfail(r, "loopback event", e);
        if (!me.consumed[slot] && (e = hipEventCreateWithFlags(&me.consumed[slot], hipEventDisableTiming)) != hipSuccess) return hipfail(r, "loopback event", e);
        if ((e = hipEventRecord(me.ready[slot], s)) != hipSuccess) return hipfail(r, "loopback record", e);
        for (int f = 0; f < nf; ++f) { me.send_s[slot][f] = rows(f).send_s; me.send_n[slot][f] = rows(f).send_n; }
        me.bytes[slot] = bytes; me.nf[slot] = nf;
        me.seq = k;
    }
    h.cv.notify_all();
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::duration<double>(h.timeout_s);
    auto wait_for = [&](auto pred, const char *what) {
        std::unique_lock<std::mutex> lk(h.mu);
        if (!h.cv.wait_until(lk, deadline, pred)) {
            r->err = std::string("loopback exchange ") + std::to_string(k) + " of rank " + std::to_string(r->rank) + ": " + what +
                     " (every ring of the hub must be driven from its own host thread, and all of them must make the same calls)";
            return false;
        }
        return true;
    };
    // (2) receives: my south halo <- the south neighbour's northern edge rows; my north halo <- the north neighbour's southern ones
    const int peers[2] = {r->south, r->north};
    for (int side = 0; side < 2; ++side) {
        if (!((sides >> side) & 1)) continue;
        const int p = peers[side];
        if (!wait_for([&] { return h.post[p].seq >= k; }, "a neighbour did not reach its matching exchange")) return SWMHD_ECOMM;
        hipEvent_t ready; const char *src[LoopHub::MAXF]; size_t pbytes; int pnf;
        {
            std::unique_lock<std::mutex> lk(h.mu);
            const LoopHub::Post &pp = h.post[p];
            ready = pp.ready[slot]; pbytes = pp.bytes[slot]; pnf = pp.nf[slot];
            for (int f = 0; f < nf && f < pnf; ++f) src[f] = side == 0 ? pp.send_n[slot][f] : pp.send_s[slot][f];
        }
        if (pbytes != bytes || pnf != nf) { r->err = "loopback exchange: neighbour posted a different message (fields / bytes)"; return SWMHD_ECOMM; }
        if ((e = hipStreamWaitEvent(s, ready, 0)) != hipSuccess) return hipfail(r, "loopback wait", e);
        for (int f = 0; f < nf; ++f)
            if ((e = hipMemcpyAsync(side == 0 ? rows(f).recv_s : rows(f).recv_n, src[f], bytes, hipMemcpyDeviceToDevice, s)) != hipSuccess)
                return hipfail(r, "loopback copy", e);
    }
    {   // (3) rows consumed
        std::unique_lock<std::mutex> lk(h.mu);
        LoopHub::Post &me = h.post[r->rank];
        if ((e = hipEventRecord(me.consumed[slot], s)) != hipSuccess) return hipfail(r, "loopback record", e);
        me.done = k;
    }
    h.cv.notify_all();
    // (4) my sends complete when both neighbours have taken my rows: later work on s may overwrite them
    for (int side = 0; side < 2; ++side) {
        if (!((sides >> side) & 1)) continue;
        const int p = peers[side];
        if (!wait_for([&] { return h.post[p].done >= k; }, "a neighbour did not take the rows sent to it")) return SWMHD_ECOMM;
        hipEvent_t consumed;
        { std::unique_lock<std::mutex> lk(h.mu); consumed = h.post[p].consumed[slot]; }
        if ((e = hipStreamWaitEvent(s, consumed, 0)) != hipSuccess) return hipfail(r, "loopback wait", e);
    }
    return SWMHD_OK;
}

// One exchange of the Hy edge rows of every field, enqueued on s.  sides: bit 0 = with the south neighbour, bit 1 = with the north
// one (3: the ring's full exchange; a chain leaves out its walls).  RCCL: one grouped launch -- for every field, northern edge rows ->
// north neighbour's south halo, southern edge rows -> south neighbour's north halo.  Issue order (send_n, recv_s, send_s, recv_n per
// field) is what makes the 1- and 2-rank rings, where both neighbours are the same peer, pair up correctly: RCCL matches sends and
// receives of a peer in issue order.
template <typename T>
int exchange(swmhd_ring *r, T *const *fields, int nf, const swmhd::Grid &g, hipStream_t s, int sides = 3) {
    if (!r || !fields || nf <= 0 || (sides & ~3)) return SWMHD_EINVAL;
    if (g.Nx <= 0 || g.Ny < g.Hy || g.Hy <= 0 || !g.stride_ok()) return SWMHD_EINVAL;   // (rows to send: a halo, and a slab that covers it)
    for (int f = 0; f < nf; ++f)
        if (!fields[f]) return SWMHD_EINVAL;
    if (!sides) return SWMHD_OK;
    if (r->hub && nf > LoopHub::MAXF) return SWMHD_EINVAL;
    const size_t count = (size_t)g.Hy * (size_t)g.sy;   // Hy full rows (the pitch padding of the last row travels too: harmless)
    auto rows = [&](int f) { return edge_rows(fields[f], g.Ny, g.Hy, g.sy); };
    if (r->hub) return loopback_exchange(r, rows, nf, count * sizeof(T), sides, s);
    ncclResult_t rc = r->api.GroupStart();
    if (rc != ncclSuccess) return fail(r, "ncclGroupStart", rc);
    const bool so = sides & 1, n = sides & 2;
    for (int f = 0; f < nf; ++f) {
        const EdgeRows e = rows(f);
        if (n && (rc = r->api.Send(e.send_n, count, nccl_type<T>(), r->north, r->comm, s)) != ncclSuccess) break;
        if (so && (rc = r->api.Recv(e.recv_s, count, nccl_type<T>(), r->south, r->comm, s)) != ncclSuccess) break;
        if (so && (rc = r->api.Send(e.send_s, count, nccl_type<T>(), r->south, r->comm, s)) != ncclSuccess) break;
        if (n && (rc = r->api.Recv(e.recv_n, count, nccl_type<T>(), r->north, r->comm, s)) != ncclSuccess) break;
    }
    ncclResult_t rc2 = r->api.GroupEnd();
    if (rc != ncclSuccess) return fail(r, "ncclSend/ncclRecv", rc);
    if (rc2 != ncclSuccess) return fail(r, "ncclGroupEnd", rc2);
    return SWMHD_OK;
}

// Stream `to` waits for what stream `from` has enqueued so far, through the ring's event of that direction (ev_main: main -> comm,
// ev_comm: comm -> main).
hipError_t follow(hipStream_t to, hipStream_t from, hipEvent_t ev) {
    const hipError_t e = hipEventRecord(ev, from);
    return e == hipSuccess ? hipStreamWaitEvent(to, ev, 0) : e;
}

// Drain the exchange in flight (if any): `s` waits for the comm stream.
int join(swmhd_ring *r, hipStream_t s) {
    if (!r->pending) return SWMHD_OK;
    if (hipError_t e = follow(s, r->comm_stream, r->ev_comm)) return hipfail(r, "join", e);
    r->pending = nullptr;
    return SWMHD_OK;
}

// One call of a slab driver (swmhd_ring_step_rk3 and _bc): nsteps RK3 steps of one y-slab by one of two schedules, the deep-halo one
// (described below) or the per-stage one.  Per stage (X = current state, Y = the other buffer set; cut sides: those whose halo rows
// come from a neighbour -- both of a ring's slab, the sides without a wall of a chain's):
//   main stream : rows of X that need no remote data -> Y: the interior, and the Hy-row strip of a wall side (the exchange of X is
//                 still in flight)
//   comm stream : ... exchange of X ... ; the Hy-row strips of the cut sides of X -> Y     (one launch, queued behind the exchange)
//   no fill     : comm: exchange of Y straight after the strips ; comm waits for main's interior ; main waits for the strips
//   a fill      : main: wait(comm) ; fill of Y ; comm waits ; comm: exchange of Y   (x halos live in memory: corners travel with rows)
// The fill is none (periodic, x wrapped on read), the periodic x fill, or a Bounded slab's boundary-condition fill (x, and the wall
// sides).  Either way the exchange of Y overlaps the next stage's interior rows.  A thin slab is bound by the chain exchange -> strips
// -> exchange on the comm stream (tools/ring_rehearsal.py), which is why that chain has no hop through the main stream when no fill
// runs.  A chain of one has no cut and exchanges nothing.  The first stage of a call that finds no exchange in flight (the caller's
// halos current) runs all rows at once on the main stream.
template <typename T>
struct Slab {
    swmhd_ring *r;
    hipStream_t s, c;   // the caller's stream (main) and, from begin() on, the ring's comm stream
    swmhd::Rk3Buffers<T> b;
    swmhd::Grid g;
    swmhd::Physics<T> ph;   // the model and dt; run() adds the stage's scalars
    bool anchor;   // fast periodic slabs: the anchor form, 96 B/cell in every stage (common.hpp: Rk3Buffers); else the G- form
    int *state_in_alt;

    // rows [j0, j1) and [j0b, j1b) of stage g on stream `on`
    int run(const swmhd::Rk3Stage<T> &sg, int j0, int j1, int j0b, int j1b, int fl, hipStream_t on) {
        swmhd::Physics<T> st = ph;
        st.gamma = sg.gamma; st.zeta = sg.zeta; st.store_G = sg.store_G;
        return swmhd::tendencies_rk3<T>(b.cur, b.alt, b.gn, sg.Gm, g, st, swmhd::Rows{j0, j1, j0b, j1b}, fl | sg.flags, (void *)on);
    }
    // checks of both drivers, before any HIP call or read of the ring: the first stage's over an empty row range, and the fill's own
    int check(T *const *q, T *const *q_alt, T *const *Ga, T *const *Gb, int flags) {
        if (g.Ny < 2 * g.Hy + 1) return SWMHD_EINVAL;   // a slab needs interior rows between its two strips
        if (!b.set(q, q_alt, Ga, Gb)) return SWMHD_EINVAL;
        if (int rc = run(b.stage(0, anchor), 0, 0, 0, 0, flags, s)) return rc;
        return g.Hx > g.Nx ? SWMHD_EHALO : SWMHD_OK;
    }
    // drain an exchange in flight for another state; what the caller enqueued so far precedes all this call puts on the comm stream
    int begin() {
        c = r->comm_stream;
        if (r->pending != (const void *)b.cur[0])
            if (int rc = join(r, s)) return rc;
        return comm_waits();
    }
    // exit: after an error whatever was enqueued stays enqueued, so order the caller's stream behind the comm stream and forget the
    // exchange in flight (`pending` never describes one not fully issued); tell the caller which set holds the newest completed stage
    int end(int rc) {
        if (rc) { (void)follow(s, c, r->ev_comm); r->pending = nullptr; }
        if (state_in_alt) *state_in_alt = b.swaps & 1;
        return rc;
    }
    int comm_waits() { const hipError_t e = follow(c, s, r->ev_main); return e == hipSuccess ? SWMHD_OK : hipfail(r, "comm waits for main", e); }
    int main_waits() { const hipError_t e = follow(s, c, r->ev_comm); return e == hipSuccess ? SWMHD_OK : hipfail(r, "main waits for comm", e); }
    int exchange_cur(int cuts) {
        const int rc = exchange<T>(r, b.cur, 4, g, c, cuts);
        if (!rc) r->pending = b.cur[0];
        return rc;
    }
    // the interior launch of a stage on the main stream, between two timing events while swmhd_ring_time_launches asks for them
    // (timing-only events: without the system-scope fence a default event performs when it is recorded -- with the comm stream's
    //  kernels running beside the interior launch that fence cost 16 % of the step, 1.53 vs 1.32 ms)
    int run_interior(const swmhd::Rk3Stage<T> &sg, int j0, int j1, int fl) {
        if (r->t0.size() >= r->tcap) return run(sg, j0, j1, 0, 0, fl, s);
        hipEvent_t t0 = nullptr, t1 = nullptr;
        hipError_t e;
        if ((e = hipEventCreateWithFlags(&t0, hipEventDisableSystemFence)) != hipSuccess) return hipfail(r, "hipEventCreate", e);
        if ((e = hipEventCreateWithFlags(&t1, hipEventDisableSystemFence)) != hipSuccess) { (void)hipEventDestroy(t0); return hipfail(r, "hipEventCreate", e); }
        (void)hipEventRecord(t0, s);
        const int rc = run(sg, j0, j1, 0, 0, fl, s);
        if (rc) { (void)hipEventDestroy(t0); (void)hipEventDestroy(t1); return rc; }
        (void)hipEventRecord(t1, s);
        r->t0.push_back(t0); r->t1.push_back(t1); r->trows.push_back(j1 - j0);
        return SWMHD_OK;
    }

    // ---- per-stage schedule.  cuts: bit 0 south, bit 1 north.  The fill follows from the flags: Bounded slabs the boundary-
    //      condition fill (gradient: device table of 16 values, or NULL), x halos in memory the periodic x fill, x wrapped on read none
    int per_stage(int nsteps, int fl, int cuts, const T *gradient) {
        const bool walls = fl & (SWMHD_BOUNDED_X | SWMHD_BOUNDED_Y), fill = walls || !(fl & SWMHD_WRAP_X);
        const swmhd::BcSides sides{swmhd::decode_flags(fl).topo_x, SWMHD_BOUNDED, swmhd::FACE_X, swmhd::FACE_Y};
        const int Ny = g.Ny, lo = (cuts & 1) ? g.Hy : 0, hi = (cuts & 2) ? Ny - g.Hy : Ny;   // rows [lo, hi) need no remote data
        for (int n = 0; n < nsteps; ++n)
            for (int st = 0; st < 3; ++st) {
                const swmhd::Rk3Stage<T> sg = b.stage(st, anchor);
                const bool split = r->pending != nullptr;
                int rc;
                // (interior rows: leave a few workgroup slots free, or the exchange and the strips could not start before it ends)
                if ((rc = split ? run_interior(sg, lo, hi, fl | SWMHD_LEAVE_ROOM) : run_interior(sg, 0, Ny, fl))) return rc;
                // the cut strips in one launch: they sit on the exchange -> strips -> exchange chain that bounds a thin slab
                if (split && ((rc = lo > 0 ? run(sg, 0, lo, hi, Ny, fl, c) : run(sg, hi, Ny, 0, 0, fl, c)) || (rc = main_waits()))) return rc;
                b.rotate();
                r->pending = nullptr;   // the exchange of the OLD state has been consumed; none of the new state is in flight yet
                if (split && !fill) {
                    // The rows the exchange sends are exactly the strips' output and no fill touches them: the exchange of the new
                    // state follows the strips on the comm stream directly, without a round trip through the main stream; only the
                    // NEXT stage's strips wait for this stage's interior rows.
                    if ((rc = exchange_cur(cuts)) || (rc = comm_waits())) return rc;
                    continue;
                }
                if (walls && (rc = swmhd::fill_halo_walls<T>(b.cur, 4, g, sides, 3 & ~cuts, nullptr, gradient, (void *)s))) return rc;
                if (!walls && fill && (rc = swmhd::fill_halo_periodic_multi<T>(b.cur, 4, g, SWMHD_HALO_X, (void *)s))) return rc;
                if (!cuts) continue;   // a chain of one: both walls local, nothing to exchange
                if ((rc = comm_waits()) || (rc = exchange_cur(cuts))) return rc;
            }
        return SWMHD_OK;
    }

    // ---- deep-halo schedule: ONE exchange per step instead of one per stage (periodic rings) ------------------------------------
    // With Hy >= 9 a slab evaluates the rows of its neighbours it needs for stages 2 and 3 itself (redundantly: 18 extra rows
    // per step) from the 9 halo rows exchanged once per step.  Rows per stage (north side mirrored):
    //     stage 1   interior [3, Ny-3)     boundary [-6, 3)      stage 2   interior [9, Ny-9)    boundary [-3, 9)
    //     stage 3   interior [12, Ny-12)   boundary [0, 12)
    // Interior launches (main stream) read only what earlier interior launches of the same step wrote -- plus, for stage 1,
    // the boundary rows of the previous step's last stage: ONE wait of the main stream per step.  Boundary launches (comm
    // stream, behind the exchange) read rows of the previous interior launch: the comm stream waits twice, off the critical
    // path.  Stage 2's interior starts at row 9, not 6, because it overwrites the buffer whose rows [0, 9) the exchange in
    // flight is still sending.  A thin slab (strong scaling) is then bound by its interior launches, not by the chain
    // exchange -> strips -> exchange of the per-stage schedule (tools/ring_rehearsal.py).
    int deep_halo(int nsteps, int flags) {
        const int ilo[3] = {3, 9, 12}, blo[3] = {-6, -3, 0};
        // boundary zones of a wide slab take the row-marching kernel too (both zones in one launch, a few dozen workgroups beside the
        // interior launch); the LDS-tiled kernel re-loads a 10-row halo per 4-row tile and costs ten times as much per row
        const int bflags = flags | ((!(flags & (SWMHD_STRICT | SWMHD_TILE_KERNEL | SWMHD_MARCH_KERNEL)) && g.Nx >= 1024) ? SWMHD_MARCH_KERNEL : 0);
        const int Ny = g.Ny;
        int rc;
        for (int n = 0; n < nsteps; ++n) {
            for (int st = 0; st < 3; ++st) {
                const swmhd::Rk3Stage<T> sg = b.stage(st, anchor);
                if ((rc = run_interior(sg, ilo[st], Ny - ilo[st], flags | SWMHD_LEAVE_ROOM))) return rc;
                // boundary rows of this stage, both sides in one launch, behind the exchange (stage 1) / the previous boundary launch
                if ((rc = run(sg, blo[st], ilo[st], Ny - ilo[st], Ny - blo[st], bflags, c))) return rc;
                if (st < 2 && (rc = comm_waits())) return rc;   // the next boundary launch reads rows of this interior launch
                b.rotate();
            }
            // end of the step: the main stream's next interior launch reads the last boundary rows; the exchange of the new state
            // (its 9 edge rows are exactly those boundary rows) follows them on the comm stream
            r->pending = nullptr;
            if ((rc = main_waits()) || (rc = exchange_cur(3))) return rc;
        }
        return SWMHD_OK;
    }
};

// swmhd_ring_step_rk3: a periodic ring -- both sides cut, stages in anchor form (fast) or G- form (strict)
template <typename T>
int ring_step(swmhd_ring *r, T *const *q, T *const *q_alt, T *const *Ga, T *const *Gb, const swmhd::Grid &g, const swmhd::Physics<T> &ph,
              int nsteps, int flags, int *state_in_alt, void *stream) {
    if (!r || !q || !q_alt || !Ga || !Gb || nsteps < 0) return SWMHD_EINVAL;
    if (flags & (SWMHD_BOUNDED_X | SWMHD_BOUNDED_Y)) return SWMHD_ENOTSUP;   // walls: swmhd_ring_step_rk3_bc (its fill is the BC fill)
    if (flags & SWMHD_WRAP_Y) return SWMHD_EINVAL;   // y images belong to the neighbours (x may be wrapped on read: no x-halo kernel then)
    Slab<T> x{r, (hipStream_t)stream, nullptr, {}, g, ph, !(flags & SWMHD_STRICT), state_in_alt};
    if (int rc = x.check(q, q_alt, Ga, Gb, flags)) return rc;
    if (nsteps == 0) return x.end(SWMHD_OK);
    if (int rc = x.begin()) return rc;
    const bool deep = (flags & SWMHD_WRAP_X) && g.Hy >= 9 && g.Ny >= 32;
    return x.end(deep ? x.deep_halo(nsteps, flags) : x.per_stage(nsteps, flags, 3, nullptr));
}

// swmhd_ring_step_rk3_bc: Bounded slabs, stages in G- form (as the single Bounded model), the per-stage schedule with the boundary-
// condition fill.  With SWMHD_BOUNDED_Y the ranks form a CHAIN -- rank 0 holds the south wall, the last rank the north wall, every
// other side is a cut to a neighbour; with SWMHD_BOUNDED_X alone a periodic-y ring whose x walls are local to every slab.
template <typename T>
int ring_step_bc(swmhd_ring *r, T *const *q, T *const *q_alt, T *const *Ga, T *const *Gb, const swmhd::Grid &g, const swmhd::Physics<T> &ph,
                 int nsteps, const T *gradient, int flags, int *state_in_alt, void *stream) {
    if (flags & ~(swmhd::RING_BC_FLAGS | swmhd::RING_BC_NOTSUP)) return SWMHD_EINVAL;
    if (!(flags & swmhd::BOUNDED_FLAGS)) return SWMHD_EINVAL;   // periodic slabs: swmhd_ring_step_rk3
    if (flags & swmhd::RING_BC_NOTSUP) return SWMHD_ENOTSUP;
    if ((flags & SWMHD_WRAP_Y) || swmhd::bounded_wrap_conflict(flags)) return SWMHD_EINVAL;   // y images belong to the neighbours
    if (!r || !q || !q_alt || !Ga || !Gb || nsteps < 0) return SWMHD_EINVAL;
    Slab<T> x{r, (hipStream_t)stream, nullptr, {}, g, ph, false, state_in_alt};
    if (int rc = x.check(q, q_alt, Ga, Gb, flags)) return rc;   // (the SWMHD_OPEN_* bits set below change none of its checks)
    if (nsteps == 0) return x.end(SWMHD_OK);
    const bool chain = flags & SWMHD_BOUNDED_Y;
    const int walls_y = chain ? (r->rank == 0 ? 1 : 0) | (r->rank == r->nranks - 1 ? 2 : 0) : 0, cuts = 3 & ~walls_y;
    const int fl = flags | (chain && (cuts & 1) ? SWMHD_OPEN_SOUTH : 0) | (chain && (cuts & 2) ? SWMHD_OPEN_NORTH : 0);
    if (int rc = x.begin()) return rc;
    return x.end(x.per_stage(nsteps, fl, cuts, gradient));
}

// rank `rank` of `nranks` with its neighbours, its comm stream (the device's highest priority) and its two events
hipError_t init_ring(swmhd_ring *r, int nranks, int rank) {
    r->nranks = nranks; r->rank = rank;
    r->south = (rank + nranks - 1) % nranks; r->north = (rank + 1) % nranks;
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);   // hi = numerically lowest = highest priority
    hipError_t e = hipStreamCreateWithPriority(&r->comm_stream, hipStreamNonBlocking, hi);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->ev_main, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->ev_comm, hipEventDisableTiming);
    return e;
}

}  // namespace

extern "C" {

int swmhd_ring_available(const char *rccl_path) {
    RcclApi api;
    std::string err;
    return load_rccl(rccl_path, api, err) ? SWMHD_OK : SWMHD_ENOTSUP;
}

int swmhd_ring_unique_id(const char *rccl_path, void *id128) {
    if (!id128) return SWMHD_EINVAL;
    RcclApi api;
    std::string err;
    if (!load_rccl(rccl_path, api, err)) return SWMHD_ENOTSUP;
    ncclUniqueId id;
    if (api.GetUniqueId(&id) != ncclSuccess) return SWMHD_ECOMM;
    static_assert(sizeof(id) == SWMHD_RING_ID_BYTES, "ncclUniqueId size");
    memcpy(id128, &id, sizeof(id));
    return SWMHD_OK;   // (the dlopen handle is deliberately kept: the library stays loaded for swmhd_ring_create)
}

int swmhd_ring_create(swmhd_ring **out, const char *rccl_path, int nranks, int rank, const void *id128) {
    if (!out || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return SWMHD_EINVAL;
    swmhd_ring *r = new (std::nothrow) swmhd_ring;
    if (!r) return SWMHD_EINVAL;
    if (!load_rccl(rccl_path, r->api, r->err)) { delete r; return SWMHD_ENOTSUP; }
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    if (r->api.CommInitRank(&r->comm, nranks, id, rank) != ncclSuccess) { delete r; return SWMHD_ECOMM; }
    if (hipError_t e = init_ring(r, nranks, rank)) { swmhd_ring_destroy(r); return swmhd::hiprc(e); }
    *out = r;
    return SWMHD_OK;
}

int swmhd_ring_create_loopback(swmhd_ring **out, int nranks, double timeout_s) {
    if (!out || nranks < 1 || nranks > 64) return SWMHD_EINVAL;
    std::shared_ptr<LoopHub> hub;
    try { hub = std::make_shared<LoopHub>(nranks); } catch (...) { return SWMHD_EINVAL; }
    if (timeout_s > 0) hub->timeout_s = timeout_s;
    for (int k = 0; k < nranks; ++k) out[k] = nullptr;
    for (int k = 0; k < nranks; ++k) {
        swmhd_ring *r = new (std::nothrow) swmhd_ring;
        hipError_t e = hipErrorOutOfMemory;
        if (r) { r->hub = hub; e = init_ring(r, nranks, k); }
        if (e != hipSuccess) {
            if (r) swmhd_ring_destroy(r);
            for (int j = 0; j < k; ++j) { swmhd_ring_destroy(out[j]); out[j] = nullptr; }
            return -(int)e;
        }
        out[k] = r;
    }
    return SWMHD_OK;
}

int swmhd_ring_destroy(swmhd_ring *r) {
    if (!r) return SWMHD_OK;
    if (r->comm_stream) (void)hipStreamSynchronize(r->comm_stream);
    for (auto ev : r->t0) (void)hipEventDestroy(ev);
    for (auto ev : r->t1) (void)hipEventDestroy(ev);
    if (r->comm) r->api.CommDestroy(r->comm);
    if (r->ev_main) (void)hipEventDestroy(r->ev_main);
    if (r->ev_comm) (void)hipEventDestroy(r->ev_comm);
    if (r->comm_stream) (void)hipStreamDestroy(r->comm_stream);
    delete r;
    return SWMHD_OK;
}

const char *swmhd_ring_last_error(const swmhd_ring *r) { return r ? r->err.c_str() : "null ring"; }

void *swmhd_ring_comm_stream(const swmhd_ring *r) { return r ? (void *)r->comm_stream : nullptr; }

int swmhd_ring_join(swmhd_ring *r, void *stream) { return r ? join(r, (hipStream_t)stream) : SWMHD_EINVAL; }

int swmhd_ring_time_launches(swmhd_ring *r, int max_launches) {
    if (!r || max_launches < 0) return SWMHD_EINVAL;
    for (auto ev : r->t0) (void)hipEventDestroy(ev);
    for (auto ev : r->t1) (void)hipEventDestroy(ev);
    r->t0.clear(); r->t1.clear(); r->trows.clear();
    r->tcap = (size_t)max_launches;
    return SWMHD_OK;
}

int swmhd_ring_launch_times(swmhd_ring *r, float *ms, int *rows, int capacity) {
    if (!r || !ms || !rows) return -1;
    int n = 0;
    for (size_t i = 0; i < r->t0.size() && n < capacity; ++i) {
        if (hipEventSynchronize(r->t1[i]) != hipSuccess) break;
        if (hipEventElapsedTime(&ms[n], r->t0[i], r->t1[i]) != hipSuccess) break;
        rows[n++] = r->trows[i];
    }
    return n;
}

#define SWMHD_DEF_RING(sfx, T)                                                                                                   \
    int swmhd_ring_exchange_y_##sfx(swmhd_ring *r, T *const *fields, int nfields, int Nx, int Ny, int Hx, int Hy, int64_t sy,    \
                                    void *stream) {                                                                              \
        return exchange<T>(r, fields, nfields, swmhd::Grid{Nx, Ny, Hx, Hy, sy}, (hipStream_t)stream);                            \
    }                                                                                                                            \
    int swmhd_ring_exchange_y_sides_##sfx(swmhd_ring *r, T *const *fields, int nfields, int Nx, int Ny, int Hx, int Hy,          \
                                          int64_t sy, int sides, void *stream) {                                                 \
        return exchange<T>(r, fields, nfields, swmhd::Grid{Nx, Ny, Hx, Hy, sy}, (hipStream_t)stream, sides);                     \
    }                                                                                                                            \
    int swmhd_ring_step_rk3_##sfx(swmhd_ring *r, T *const *q, T *const *q_alt, T *const *Ga, T *const *Gb, int Nx, int Ny,       \
                                  int Hx, int Hy, int64_t sy, T dx, T dy, T g, T f, int formulation, int lorentz, T dt,          \
                                  int nsteps, int flags, int *state_in_alt, void *stream) {                                      \
        swmhd::Physics<T> ph{g, f, formulation, lorentz};                                                                        \
        ph.dt = dt;                                                                                                              \
        return ring_step<T>(r, q, q_alt, Ga, Gb, swmhd::Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, nsteps, flags, state_in_alt, stream); \
    }                                                                                                                            \
    int swmhd_ring_step_rk3_bc_##sfx(swmhd_ring *r, T *const *q, T *const *q_alt, T *const *Ga, T *const *Gb, int Nx, int Ny,    \
                                     int Hx, int Hy, int64_t sy, T dx, T dy, T g, T f, int formulation, int lorentz, T dt,       \
                                     int nsteps, const T *gradient, int flags, int *state_in_alt, void *stream) {               \
        swmhd::Physics<T> ph{g, f, formulation, lorentz};                                                                        \
        ph.dt = dt;                                                                                                              \
        return ring_step_bc<T>(r, q, q_alt, Ga, Gb, swmhd::Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, nsteps, gradient, flags,        \
                               state_in_alt, stream);                                                                            \
    }

SWMHD_DEF_RING(f64, double)
SWMHD_DEF_RING(f32, float)

}  // extern "C"
