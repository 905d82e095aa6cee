/* ll_kf_list.h -- the vocabulary of "a list of frames of an ll_keyframes store, each under a given or its stored pose", once:
 * ll_visibility_run, ll_entropy_run, ll_bev_match (target and query side) and the keyframe inserts of ll_map_merge.hip all take
 * such lists, refuse the same things with the same words and find the frames' clouds in the pool the same way.
 *   LLKfList     one list: ids, poses (NULL: the stored ones), and the side's name in the messages (BEV's "target" / "query");
 *   llkf_pose    the pose of list entry f;
 *   llkf_cloud   a frame's cloud of type w: its first point in the pool (region 1 begins at cap0) and its count;
 *   llkf_check   a list against the store's table: ids inside the store, duplicates under the caller's policy, finite poses --
 *                the first error in list order wins --, and the list's point total.
 * What differs per site stays there: the empty / NULL-list message, the capacity checks, the device segment structs.
 * Plain C++ over the table, not the store: tests/native/kf_list_host.cpp includes nothing of the library but this header. */
#pragma once
#include "lightloam_hip.h"
#include <string>
#include <vector>

struct LLKfList { int n; const int *ids; const double *poses; const char *side; };   /* side: "" for everyone but BEV */
struct LLKfCloud { long long off; int cnt; };
enum LLKfDup { LLKF_DUP_ALLOWED, LLKF_DUP_PER_OP, LLKF_DUP_PER_CALL };              /* may an id repeat? if not: inside what */

static inline const double *llkf_pose(const ll_keyframe_info *tab, const LLKfList &l, int f)
{
    return l.poses ? l.poses + (size_t)f * 7 : tab[l.ids[f]].pose_w7;
}

static inline LLKfCloud llkf_cloud(const ll_keyframe_info *tab, long long cap0, int id, int w)
{
    return {(w ? cap0 : 0) + tab[id].offset[w], tab[id].n[w]};
}

/* LL_OK and *points = the points of the listed frames, or LL_ERR_ARG and *msg = who + what is wrong with the first bad entry.
 * seen: one int per frame of the store, -1 before a call's first list (not read under LLKF_DUP_ALLOWED, may be NULL); stamp: the
 * list's op.  Only a list that passes leaves all its ids marked: a refusal refuses the whole call */
static inline int llkf_check(const ll_keyframe_info *tab, int size, const LLKfList &l, LLKfDup dup, std::vector<int> *seen, int stamp, const std::string &who,
                             std::string *msg, long long *points)
{
    const std::string side = *l.side ? std::string(l.side) + " " : std::string();
    const int mark = dup == LLKF_DUP_PER_CALL ? 0 : stamp;
    long long total = 0;
    for (int f = 0; f < l.n; ++f) {
        const int id = l.ids[f];
        if (id < 0 || id >= size) { *msg = who + side + "frame " + std::to_string(id) + " is not in the store (size " + std::to_string(size) + ")"; return LL_ERR_ARG; }
        if (dup != LLKF_DUP_ALLOWED) {
            if ((*seen)[id] == mark) { *msg = who + "frame " + std::to_string(id) + " is listed twice in this " + (dup == LLKF_DUP_PER_CALL ? "call" : "op"); return LL_ERR_ARG; }
            (*seen)[id] = mark;
        }
        const double *P = llkf_pose(tab, l, f);
        for (int k = 0; k < 7; ++k)
            if (!__builtin_isfinite(P[k])) { *msg = who + "the pose of " + side + "list entry " + std::to_string(f) + " is not finite"; return LL_ERR_ARG; }
        total += (long long)tab[id].n[0] + tab[id].n[1];
    }
    *points = total;
    return LL_OK;
}
