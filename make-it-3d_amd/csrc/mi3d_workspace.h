// The workspace layouts of the mesh units (mesh.hip, meshclean.hip, meshsimplify.hip, meshsmooth.hip, meshcollapse.hip),
// each stated ONCE: a layout function walks its arrays with a Walker, and the same walk gives the pointers (on the
// caller's base) and the size the *_workspace query reports (on a null base, see bytes_of).  A size formula and a carve
// that disagree would be an out-of-bounds write on the device; here there is nothing to disagree.
//
// Host only, plain C++17, no HIP include: the system compiler builds it alone (tests/workspace_walk.cpp does, under
// AddressSanitizer).  Every array is padded to 8 bytes but the last one of marching cubes, whose size the ABI fixed
// before.  Workgroups are kLayoutBlock threads in every unit that has a row of block sums here.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mi3d_workspace {

constexpr uint32_t kLayoutBlock = 256;

inline uint32_t blocks_of(uint32_t n, uint32_t block) { return (n + block - 1) / block; }

inline size_t pad8(size_t b) { return (b + 7) / 8 * 8; }

// A byte cursor over `base`; on a null base every pointer is null and only the offset counts.
class Walker {
public:
    explicit Walker(void *base) : base_(static_cast<char *>(base)) {}
    // `count` elements of T from here on; the cursor moves on by their bytes, padded to 8 unless the layout's size
    // never had the padding (`padded` false: the last array of marching cubes)
    template <typename T>
    T *take(size_t count, bool padded = true) {
        T *p = base_ ? reinterpret_cast<T *>(base_ + offset_) : nullptr;
        offset_ += padded ? pad8(count * sizeof(T)) : count * sizeof(T);
        return p;
    }
    size_t offset() const { return offset_; }

private:
    char *base_;
    size_t offset_ = 0;
};

// a layout over the caller's workspace, and the bytes the same walk takes
template <typename Layout, typename... Sizes>
auto at(void *ws, Layout layout, Sizes... sizes) {
    Walker p(ws);
    return layout(p, sizes...);
}

template <typename Layout, typename... Sizes>
size_t bytes_of(Layout layout, Sizes... sizes) {
    Walker p(nullptr);
    layout(p, sizes...);
    return p.offset();
}

struct McWorkspace {
    unsigned long long *block_t;  // triangle sums / offsets per workgroup
    uint32_t *block_v;            // vertex sums / offsets per workgroup
    uint32_t *first_id;           // first vertex id per grid point: not padded
};

inline McWorkspace mc_layout(Walker &p, uint32_t n) {
    const uint32_t nb = blocks_of(n, kLayoutBlock);
    return {p.take<unsigned long long>(nb), p.take<uint32_t>(nb), p.take<uint32_t>(n, false)};  // in this order
}

struct CleanWorkspace {
    uint32_t *block_v, *block_t;  // kept vertices / triangles per workgroup, then their offsets
    uint8_t *flag;                // keep flag per vertex, meaningful at label rows
};

inline CleanWorkspace clean_layout(Walker &p, uint32_t nv, uint32_t nt) {
    return {p.take<uint32_t>(blocks_of(nv, kLayoutBlock)), p.take<uint32_t>(blocks_of(nt, kLayoutBlock)), p.take<uint8_t>(nv)};
}

struct SimplifyWorkspace {
    int32_t *table_v, *table_t;                           // cluster and duplicate tables   <- filled with -1
    unsigned long long *acc;                              // S and n per vertex: [nv][4]    <- zeroed, with
    uint8_t *ref;                                         // the reference mark per vertex
    int32_t *lead, *tslot;                                // [nv], [nt]
    uint32_t *block_v, *block_t;                          // emitted vertices / surviving triangles per workgroup, offsets
    uint32_t *clusters_v, *degenerate_t, *duplicate_t;    // per workgroup
    uint32_t cap_v, cap_t;                                // powers of two, at most 2^31
    unsigned long long fill_words;                        // 8-byte words of the -1 region
    unsigned long long zero_words;                        // 8-byte words of the zeroed region behind it
};

// the smallest power of two above n, shifted by `shift`, at most 2^31 (slots are int32)
inline unsigned long long simplify_capacity(unsigned long long n, int shift) {
    unsigned long long p = 1;
    while (p <= n) p <<= 1;
    p <<= shift;
    return p > (1ull << 31) ? (1ull << 31) : p;
}

// shift 1: the recommended table size, 0: the tight one
inline SimplifyWorkspace simplify_layout(Walker &p, uint32_t nv, uint32_t nt, int shift) {
    const uint32_t nbv = blocks_of(nv, kLayoutBlock), nbt = blocks_of(nt, kLayoutBlock);
    SimplifyWorkspace w;
    w.cap_v = (uint32_t)simplify_capacity(nv, shift);
    w.cap_t = (uint32_t)simplify_capacity(nt, shift);
    w.table_v = p.take<int32_t>(w.cap_v);
    w.table_t = p.take<int32_t>(w.cap_t);
    w.fill_words = p.offset() / 8;
    w.acc = p.take<unsigned long long>((size_t)nv * 4);
    w.ref = p.take<uint8_t>(nv);
    w.zero_words = p.offset() / 8 - w.fill_words;
    w.lead = p.take<int32_t>(nv);
    w.tslot = p.take<int32_t>(nt);
    w.block_v = p.take<uint32_t>(nbv);
    w.block_t = p.take<uint32_t>(nbt);
    w.clusters_v = p.take<uint32_t>(nbv);
    w.degenerate_t = p.take<uint32_t>(nbt);
    w.duplicate_t = p.take<uint32_t>(nbt);
    return w;
}

struct alignas(8) IndexPair {  // the other two corners of a triangle at a vertex
    int32_t x, y;
};

struct SmoothWorkspace {
    int32_t *cur;           // degree, then cursor, per vertex
    uint32_t *offs, *block; // [nv + 1], [blocks of nv]
    uint8_t *moves;         // [nv]
    float *tmp;             // the second vertex buffer: [nv][3]
    IndexPair *pairs;       // [3 nt]
};

inline SmoothWorkspace smooth_layout(Walker &p, uint32_t nv, uint32_t nt) {
    SmoothWorkspace w;
    w.cur = p.take<int32_t>(nv);
    w.offs = p.take<uint32_t>((size_t)nv + 1);
    w.block = p.take<uint32_t>(blocks_of(nv, kLayoutBlock));
    w.moves = p.take<uint8_t>(nv);
    w.tmp = p.take<float>((size_t)nv * 3);
    w.pairs = p.take<IndexPair>((size_t)nt * 3);
    return w;
}

// what the rounds keep between kernels
struct CollapseCtrl {
    uint32_t live;          // live triangles at the start of the round
    uint32_t live_next;     // summed by k_co_rename
    uint32_t active;        // this round runs
    uint32_t quota;         // winners applied at most
    uint32_t round;         // r of the key's hash: the rounds run before this one
    uint32_t winners;       // of this round
    uint32_t last_winners;  // of the last round that ran (1 before the first)
    uint32_t planeless;     // usable triangles with s == 0 or a non-finite s
    uint32_t pad[8];
};

struct CollapseWorkspace {
    CollapseCtrl *ctrl;
    double *Q;                   // [nv][10]
    unsigned long long *claim;   // [nv]
    unsigned long long *keys;    // [3 nt]
    float *P;                    // [nv][3]
    int32_t *rep, *cur;          // [nv]
    uint32_t *offs, *blockv;     // [nv + 1], [blocks of nv]
    int32_t *tri;                // [nt][3]: the corners as renamed so far
    uint32_t *rows;              // [3 nt]: 3 t + k for every live triangle t with v at corner k
    float *xstar;                // [3 nt][3]
    uint32_t *blockt;            // [blocks of nt]
    uint8_t *locked, *alive, *wins;
};

inline CollapseWorkspace collapse_layout(Walker &p, uint32_t nv, uint32_t nt) {
    CollapseWorkspace w;
    w.ctrl = p.take<CollapseCtrl>(1);
    w.Q = p.take<double>((size_t)nv * 10);
    w.claim = p.take<unsigned long long>(nv);
    w.keys = p.take<unsigned long long>((size_t)nt * 3);
    w.P = p.take<float>((size_t)nv * 3);
    w.rep = p.take<int32_t>(nv);
    w.cur = p.take<int32_t>(nv);
    w.offs = p.take<uint32_t>((size_t)nv + 1);
    w.blockv = p.take<uint32_t>(blocks_of(nv, kLayoutBlock));
    w.tri = p.take<int32_t>((size_t)nt * 3);
    w.rows = p.take<uint32_t>((size_t)nt * 3);
    w.xstar = p.take<float>((size_t)nt * 9);
    w.blockt = p.take<uint32_t>(blocks_of(nt, kLayoutBlock));
    w.locked = p.take<uint8_t>(nv);
    w.alive = p.take<uint8_t>(nt);
    w.wins = p.take<uint8_t>(nt);
    return w;
}

}  // namespace mi3d_workspace
