// sq_elements.h -- the loop annotation of ONE structure row (Elements): which nested pair closes a listed loop, the walk of one
// loop and the type rule.  __host__ __device__ and free of HIP types: sq_elements_dev.hip runs it one loop per lane,
// tests/native/elements_host.cpp compiles it with g++ and runs it as one thread.
//
// A row is read in gap-free coordinates through an accessor `Row` with
//     int  n() const            positions of the record (gap columns removed)
//     int  partner(int g) const the partner position of g, -1: unpaired, or its pair touches a gap column and is dropped
//     int  level(int g) const   the signed pseudoknot level of g: +L opens, -L closes a pair of level L, 0 otherwise
//     bool sep(int g) const     g holds a separator
// The NESTED pairs are those of level 1; they do not cross one another (PairsToDBN's groups are conflict-free), so the loops
// they close form a tree and every position that is not in a nested pair belongs to exactly one loop.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SQ_ELEM_HD __host__ __device__ inline
#else
#define SQ_ELEM_HD inline
#endif

// the codes of ElementsResult.element; the first six are the loop types of ElementsResult.loops as well
enum {
    SQ_ELEM_EXTERIOR = 0, SQ_ELEM_STEM = 1, SQ_ELEM_HAIRPIN = 2, SQ_ELEM_BULGE = 3, SQ_ELEM_INTERNAL = 4, SQ_ELEM_MULTI = 5,
    SQ_ELEM_PK = 6, SQ_ELEM_BREAK = 7, SQ_ELEM_GAP = 8, SQ_ELEM_CODES = 9
};
#define SQ_ELEM_STACK (-1)              // sq_elem_type: a stack -- not a loop, not listed
#define SQ_ELEM_WAVES 4                 // waves (rows) of a block of the loops kernel

struct SqElemLoop { int branches, unpaired, side5, brk; };

// Does the nested pair that position g opens close a LISTED loop?  false for every other position and for a stack: the
// next position pairs, nested, with the position before the closer -- no column lies between the two pairs.
template <class Row> SQ_ELEM_HD bool sq_elem_listed(const Row &R, int g)
{
    if (R.level(g) != 1) return false;
    const int q = R.partner(g);
    return !(g + 1 < q - 1 && R.level(g + 1) == 1 && R.partner(g + 1) == q - 1);
}

// The loop that the nested pair (g, q) closes; (-1, n) is the exterior loop.  Its positions are those between g and q that no
// nested child pair encloses: a nested opener is a branch and the walk goes on behind its closer.  visit(p) is called for
// every position of the loop that is no separator, in ascending order; positions in pairs of level >= 2 count as unpaired.
template <class Row, class Visit> SQ_ELEM_HD SqElemLoop sq_elem_walk(const Row &R, int g, int q, Visit &&visit)
{
    SqElemLoop L = {0, 0, 0, 0};
    for (int p = g + 1; p < q;) {
        if (R.level(p) == 1) { L.branches++; p = R.partner(p) + 1; continue; }      // (partner(p) > p: the walk always advances)
        if (R.sep(p)) L.brk = 1;
        else { L.unpaired++; if (!L.branches) L.side5++; visit(p); }
        p++;
    }
    return L;
}

// the first rule that matches
SQ_ELEM_HD int sq_elem_type(bool exterior, const SqElemLoop &L)
{
    if (exterior || L.brk) return SQ_ELEM_EXTERIOR;                  // (a loop with a separator is a nicked loop)
    if (L.branches == 0) return SQ_ELEM_HAIRPIN;
    if (L.branches >= 2) return SQ_ELEM_MULTI;
    if (L.unpaired == 0) return SQ_ELEM_STACK;
    return L.side5 == 0 || L.side5 == L.unpaired ? SQ_ELEM_BULGE : SQ_ELEM_INTERNAL;
}
