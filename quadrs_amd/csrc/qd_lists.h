// qd_lists.h — the cursor of an event list: what the sinks whose output is a log of records (the burst list,
// qd_bursts.h; the emission list, qd_emissions.h) share.  Such a list holds a running count `found`, a capacity `cap` and the first `cap`
// records in a fixed order.  A batch's records are ranked in three steps: the pieces of the batch count theirs (`totals`), one workgroup
// turns the totals into exclusive `bases` from `found` (list_scan), and every piece stores the records whose rank, its base plus the
// records before them in the piece, is below cap.  Inside a round of 256 lanes that rank is a ballot and popcounts (list_round_rank).
//
// The first half is plain integer code, as in the two users: it compiles as C++17 on the host and under hipcc.
#ifndef QD_LISTS_H
#define QD_LISTS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define QD_LISTS_HD __host__ __device__
#else
#define QD_LISTS_HD
#endif

namespace qd {

constexpr uint32_t kListThreads = 256, kListWaves = kListThreads / 64;       // a round: the lanes of one workgroup, one candidate record each

template <typename Record>
struct ListCursor {
    unsigned long long *totals, *bases;      // per piece: the records that end in it, and the rank of the first of them
    unsigned long long *found;               // the running count
    uint64_t cap;
    Record *list;
};

// EMIT's early exit: piece q stores something iff it holds a record and its first rank (*base) has room
template <typename Record>
QD_LISTS_HD inline bool list_piece_stores(const ListCursor<Record> L, uint64_t q, uint64_t *base) {
    *base = L.bases[q];
    return L.totals[q] != 0 && *base < L.cap;
}
}  // namespace qd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace qd {

// between COUNT and EMIT: one workgroup of kListThreads turns the n pieces' totals into their bases, exclusive, from the running count,
// and adds the batch's records to it.  The cursor comes by value: the fields are the kernel's arguments, read once.
template <typename Record>
__device__ inline void list_scan(const ListCursor<Record> L, uint64_t n) {
    __shared__ unsigned long long s_sum[kListThreads];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (n + kListThreads - 1) / kListThreads;
    const uint64_t a = tid * per < n ? tid * per : n, b = a + per < n ? a + per : n;
    unsigned long long mine = 0;
    for (uint64_t q = a; q < b; ++q) mine += L.totals[q];
    s_sum[tid] = mine;
    __syncthreads();
    unsigned long long before = *L.found;
    for (uint32_t i = 0; i < tid; ++i) before += s_sum[i];
    for (uint64_t q = a; q < b; ++q) { L.bases[q] = before; before += L.totals[q]; }
    __syncthreads();
    if (tid == kListThreads - 1) *L.found = before;
}

// One round of the workgroup's 256 lanes in the list's order: the lane's record (if it keeps one) has the rank returned, rank0 being the
// rank of the round's first record; rank0 moves past the round.  s_bal holds kListWaves words; every lane of the workgroup calls this
// (one barrier inside), and the words are read until the caller's next barrier, or the next round with another s_bal.
__device__ inline uint64_t list_round_rank(bool keep, unsigned long long *s_bal, uint64_t &rank0) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const unsigned long long bal = __ballot(keep);
    if ((tid & 63u) == 0) s_bal[wave] = bal;
    __syncthreads();
    uint64_t rank = rank0;
    for (uint32_t v = 0; v < wave; ++v) rank += __popcll(s_bal[v]);
    rank += __popcll(bal & ((1ull << (tid & 63u)) - 1ull));
    for (uint32_t v = 0; v < kListWaves; ++v) rank0 += __popcll(s_bal[v]);
    return rank;
}

}  // namespace qd
#endif  // __HIPCC__
#endif
