// lu.hpp -- what lu.hip (the nested-dissection ordering, the tree, the struct lists, LUFactorization) shares with cholesky.hip
// (CholeskyFactorization: the same ordering and tree, dense panels per node) and lu_panels.hip (LUFactorization's panel form)
#pragma once
#include "amg.hpp"

namespace esplu {

constexpr u32 LU_NONE = 0xFFFFFFFFu;  // level: not placed yet; dist: not reached yet; a table without a node (n < 2^32 - 16)

// what an ordering leaves: u32 n each but anc (one u32 n per round), released on every way out unless taken over
struct Order {
    DevBuf level, root, perm, newpos, nstart, nsize, ancptr;
    std::vector<DevBuf> anc;
    i64 rounds = 0, deepest = 0, nodes = 0, launches = 0;
    ~Order() {
        for (DevBuf *b : {&level, &root, &perm, &newpos, &nstart, &nsize, &ancptr}) release(*b);
        for (DevBuf &b : anc) release(b);
    }
};

// S: struct of the node that starts at s is column s; T = transpose(S).  Both 1-based CSC arrays, nullptr when no record exists
struct Struct {
    const i64 *scp, *srv, *tcp, *trv;
};

}  // namespace esplu

#pragma GCC visibility push(hidden)
// lu.hip: the rounds of h's stored pattern (checked, square, flushed): o.level, o.anc, o.rounds, o.launches
int32_t lu_dissect(esp_handle *h, int leaf_size, int max_depth, esplu::Order &o);
// ... o.perm = the vertices sorted by (level descending, root of the node, index), o.newpos its inverse, o.root, the nodes
int32_t lu_order(esp_handle *h, esplu::Order &o);
// ... the struct lists of the ordered tree: hs.v = {S, transpose(S)} (internal handles, the caller's to keep or drop) and x their
// arrays; hs.v stays empty and x all nullptr when no node has a struct.  o.anc is rewritten to node starts.  what: the message prefix
int32_t lu_structs(esp_handle *h, esplu::Order &o, const char *what, espamg::Handles &hs, esplu::Struct &x);
// ... the argument checks of every entry point over the ordering; n values of a u32 device array into the caller's host or device
// array, as int64 (wide) or as they are
int32_t lu_check_args(esp_handle *h, const char *what, int32_t leaf_size, int32_t max_depth);
int32_t lu_export(esp_handle *h, const DevBuf &src, void *out, bool wide, int32_t on_device);
// lu_panels.hip, LUFactorization's panel form (p->lu_form == ESP_LU_PANELS): the tables and the panels' layout of the ordered tree (a
// new LuPanelData, p untouched: build_b calls it behind its last refusal); the load from B's values and the numeric factorization;
// release (ldiv! and the factor in B's position order: internal.hpp)
int32_t lup_symbolic(esp_precon *p, esplu::Order &o, espamg::Handles &hs, const esplu::Struct &x, struct LuPanelData **out);
int32_t lup_numeric(esp_precon *p);
void lup_drop(struct LuPanelData *c);
#pragma GCC visibility pop
