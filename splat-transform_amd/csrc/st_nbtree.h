// st_nbtree.h -- the search structure shared by st_neighbors.hip (the k-th-neighbour search) and
// st_clusters.hip (the fixed-radius link search): the placed rows sorted by a 30-bit Morton key, leaves
// of L consecutive sorted rows with exact boxes, an implicit 8-ary tree of boxes above them.  Built by
// build_tree (st_neighbors.hip); no result of either client depends on its shape.
#ifndef ST_NBTREE_H
#define ST_NBTREE_H

#include <string>

#include "st_internal.h"

namespace st {
namespace nbt {

constexpr int MAX_LEVELS = 12;   // leaves <= 2^30 (n < 2^32, L >= 4): at most 11 levels
constexpr int STACK = 7 * MAX_LEVELS + 8;  // a depth-first walk pushes at most 8 for one popped

struct NCols {  // kernel argument: x, y, z of any type
    const void *p[3];
    int32_t type[3];
};
struct Tree {  // kernel argument: level l's boxes are box[off[l] .. off[l] + cnt[l]) (six doubles each)
    uint32_t off[MAX_LEVELS], cnt[MAX_LEVELS];
    int levels;
};
struct Built {
    void *pos = nullptr;        // the sorted rows' positions: float4[P] when f32, double4[P] otherwise
    bool f32 = false;           // x, y and z are all float32
    uint32_t *order = nullptr;  // order[s] = the original row of sorted row s; the P placed rows first
    double *box = nullptr;      // every level's boxes, leaves first (Tree::off)
    Tree tr{};
    uint64_t nodes = 0;         // boxes of all levels together
    uint64_t P = 0;             // placed rows
    int L = 0;                  // rows per leaf
};

// the first x, y and z of the table; ST_ERR_ARG ("<what>: the table has no column z") without one
NCols xyz_cols(const st_ttable *t, const char *what);
// ST_KNN_LEAF=<4..64>, read per call; 64 otherwise
int leaf_size();
// extent, keys, radix_sort_u32_iota, gather, leaf boxes and levels of n >= 1 rows into slots under
// tag + ".nb."; waits for the stream once (the placed count).  With P = 0 there is no tree
void build_tree(st_ctx *c, const NCols &cs, uint64_t n, const std::string &tag, Built &T);

}  // namespace nbt
}  // namespace st

#endif  // ST_NBTREE_H
