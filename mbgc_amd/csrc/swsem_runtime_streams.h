// Part of swsem_runtime.hip: the process-wide pool of side streams and how a handle is dealt its four.
namespace {

// ------------------------------------------------------------------------------------------------------------------
// The side streams: a process-wide pool per device, dealt to a handle by MEASUREMENT.
// A HIP stream's hardware queue is served by one of the device's four dispatch pipes (the k-th queue a process makes
// goes to pipe k mod 4, whatever its priority: profiles/queue_pipes.hip), and a pipe works on one launch at a time: a
// kernel with more workgroups than the device holds keeps its pipe until its last workgroup has been dispatched, and a
// kernel queued meanwhile on another stream of the same pipe starts behind it. Which pipe the caller's stream sits on
// depends on how many queues its framework made before — the step time of a round moved between 2.6 and 3.0 ms with
// nothing but that (profiles/r04_stream_pipes.md). So the library makes eight candidate streams once, finds out which
// of them get in each other's way (a long-dispatch kernel on one, a one-workgroup kernel on the other), and gives every
// handle streams that do not share a pipe with its main stream or with each other where both are busy at once:
//   stream2     low     the byte automata of an emission's second phase (beside the next batch's chains, then the stitch)
//   streamAux   normal  the emission's pairing kernels (beside the insertion)
//   streamLoad  high    the finalize's copies (beside the insertion)
//   streamUp    normal  table uploads (a few microseconds at a batch's start)
// SWSEM_STREAM_CALIB=0: no measurement, the candidates in the order they were made.
struct SidePool {
    static constexpr int NC = 8;
    bool made = false, ok = false;
    hipStream_t cand[NC] = {};
    int cls[NC] = {1, 1, 1, 1, 0, 0, 2, 2};     // 0 low, 1 normal, 2 high priority
    int label[NC] = {};                          // candidates with one label get in each other's way
    unsigned wgs = 8192;
};
SidePool g_pools[16];
std::mutex g_poolMu;

double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// does a one-workgroup kernel on b wait for a long-dispatch kernel on a?
bool streams_collide(hipStream_t a, hipStream_t b, unsigned wgs) {
    int hits = 0;
    for (int rep = 0; rep < 2; rep++) {
        (void) hipStreamSynchronize(a); (void) hipStreamSynchronize(b);
        const double t0 = now_us();
        k_hog<<<dim3(wgs), dim3(256), 0, a>>>(1500);                 // 15 us per workgroup, four generations of them
        k_touch<<<1, 1, 0, b>>>();
        (void) hipStreamSynchronize(b);
        const double t1 = now_us();
        (void) hipStreamSynchronize(a);
        const double t2 = now_us();
        if (t1 - t0 > 0.6 * (t2 - t0)) hits++;
    }
    return hits == 2;
}

SidePool *side_pool(int device, int prioLow, int prioHigh, bool measure) {
    if (device < 0 || device >= 16) return nullptr;
    std::lock_guard<std::mutex> lk(g_poolMu);
    SidePool &P = g_pools[device];
    if (P.made) return P.ok ? &P : nullptr;
    P.made = true;
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0) P.wgs = (unsigned) pr.multiProcessorCount * 8u * 4u;
    for (int i = 0; i < SidePool::NC; i++) {
        const int pv = P.cls[i] == 0 ? prioLow : (P.cls[i] == 2 ? prioHigh : (prioLow + prioHigh) / 2);
        if (hipStreamCreateWithPriority(&P.cand[i], hipStreamNonBlocking, pv) != hipSuccess) return nullptr;
        k_touch<<<1, 1, 0, P.cand[i]>>>();                            // first use: the stream is given its hardware queue now
        if (hipStreamSynchronize(P.cand[i]) != hipSuccess) return nullptr;
    }
    for (int i = 0; i < SidePool::NC; i++) {
        P.label[i] = i;
        for (int j = 0; measure && j < i; j++)
            if (P.label[j] == j && streams_collide(P.cand[j], P.cand[i], P.wgs)) { P.label[i] = j; break; }
    }
    (void) hipGetLastError();
    P.ok = true;
    return &P;
}

// the handle's side streams out of the device's pool (see SidePool): by what shares a dispatch pipe with its main stream
int deal_streams(swsem *h) {
    SidePool *P = side_pool(h->device, h->prioLow, h->prioHigh, h->sw.streamCalib);
    if (!P) return fail(SWSEM_EHIP, "cannot make the side streams");
    constexpr int NC = SidePool::NC;
    bool mainHits[NC] = {};
    for (int i = 0; h->sw.streamCalib && i < NC; i++)
        if (P->label[i] == i) mainHits[i] = streams_collide(h->stream, P->cand[i], P->wgs);
    (void) hipGetLastError();
    int chosen[4] = {-1, -1, -1, -1};                                // stream2, load, aux, up
    // penalties: sharing a pipe with the main stream, with a role that is busy at the same time, being another role's stream
    const int cls[4] = {0, 2, 1, 1};
    const int clash[4][4] = {{0, 0, 0, 0}, {60, 0, 0, 0}, {60, 10, 0, 0}, {60, 0, 5, 0}};   // [role][earlier role]
    const int withMain[4] = {100, 100, 100, 20};
    for (int r = 0; r < 4; r++) {
        int best = -1, bestCost = 1 << 30;
        for (int i = 0; i < NC; i++) {
            if (P->cls[i] != cls[r]) continue;
            int cost = mainHits[P->label[i]] ? withMain[r] : 0;
            for (int q = 0; q < r; q++) {
                if (chosen[q] == i) cost += 1000;
                else if (P->label[chosen[q]] == P->label[i]) cost += clash[r][q];
            }
            if (cost < bestCost) { bestCost = cost; best = i; }
        }
        if (best < 0) return fail(SWSEM_EHIP, "no side stream of the class wanted");
        chosen[r] = best;
    }
    h->stream2 = P->cand[chosen[0]]; h->streamLoad = P->cand[chosen[1]]; h->streamAux = P->cand[chosen[2]]; h->streamUp = P->cand[chosen[3]];
    if (h->sw.streamDebug) {
        fprintf(stderr, "swsem side streams: labels");
        for (int i = 0; i < NC; i++) fprintf(stderr, " %d%s", P->label[i], mainHits[P->label[i]] ? "*" : "");
        fprintf(stderr, " (* shares the main stream's pipe); stream2 %d, load %d, aux %d, up %d\n", chosen[0], chosen[1], chosen[2], chosen[3]);
    }
    return SWSEM_OK;
}

}  // namespace
