// ycge_mesh_pool.h - the bookkeeping of the resident meshes of a scene (ycge_scene_attach_meshes / _detach_meshes, ycge_mesh_pool.cpp):
// which 32-byte units of the mesh arena's records and which mesh indices are handed out.  Pure host code without a device call, so that
// the hook ycge_debug_mesh_ranges (and a stand-alone program) can drive it with no context.
//
// The records of an upload lie in mesh order from unit 0; `end` is the first unit behind the last live range.  A range that is given back
// joins the free ranges beside it; free ranges that reach `end` move `end` back instead of being kept.  A take is first fit by address
// among the free ranges, else the range at `end`.  Mesh indices: the lowest free one, else the next; free indices at the table's end go.
#pragma once

#include <cstdint>
#include <iterator>
#include <map>
#include <set>

namespace ycge_host {

struct MeshRanges {
    std::map<uint32_t, uint32_t> free;       // first unit -> units: disjoint, never adjacent to each other or to `end`
    uint64_t end = 0;                        // units: the records' end (may pass the pool's capacity in a PLAN; the caller refuses or grows)
    std::set<int32_t> free_index;            // free mesh indices below n_index
    int32_t n_index = 0;                     // the mesh table's length
    int64_t ranges_reused = 0;

    // the first unit of a range of `units` units (0 units: a mesh without records lies nowhere - `end`, nothing taken)
    uint64_t take(uint32_t units)
    {
        if (units == 0) return end;
        for (auto it = free.begin(); it != free.end(); ++it) {
            if (it->second < units) continue;
            const uint32_t first = it->first, left = it->second - units;
            free.erase(it);
            if (left) free.emplace(first + units, left);
            ranges_reused++;
            return first;
        }
        const uint64_t first = end;
        end += units;
        return first;
    }

    void give(uint64_t first, uint32_t units)
    {
        if (units == 0) return;
        uint64_t lo = first, hi = first + units;
        auto next = free.lower_bound((uint32_t)first);
        if (next != free.begin()) {
            auto prev = std::prev(next);
            if ((uint64_t)prev->first + prev->second == lo) { lo = prev->first; free.erase(prev); }
        }
        if (next != free.end() && next->first == hi) { hi += next->second; free.erase(next); }
        if (hi == end) end = lo;
        else free.emplace((uint32_t)lo, (uint32_t)(hi - lo));
    }

    int32_t take_index()
    {
        if (!free_index.empty()) { const int32_t i = *free_index.begin(); free_index.erase(free_index.begin()); return i; }
        return n_index++;
    }

    void give_index(int32_t i)
    {
        free_index.insert(i);
        while (n_index > 0 && free_index.count(n_index - 1)) free_index.erase(--n_index);
    }
};

// the body of ycge_debug_mesh_ranges: n_ops triples {op, a, b} on one MeshRanges that starts with `end0` units of records and `n_index0`
// indices - 0: take a units, 1: give the range of b units at unit a, 2: take an index, 3: give index a.  out: per op {the take's answer
// (else 0), end, free ranges, free units}
inline void mesh_ranges_run(int64_t end0, int32_t n_index0, const int64_t *ops, int32_t n_ops, int64_t *out)
{
    MeshRanges R;
    R.end = (uint64_t)end0;
    R.n_index = n_index0;
    for (int32_t k = 0; k < n_ops; k++) {
        const int64_t op = ops[3 * k], a = ops[3 * k + 1], b = ops[3 * k + 2];
        int64_t res = 0;
        if (op == 0) res = (int64_t)R.take((uint32_t)a);
        else if (op == 1) R.give((uint64_t)a, (uint32_t)b);
        else if (op == 2) res = R.take_index();
        else if (op == 3) R.give_index((int32_t)a);
        int64_t free_units = 0;
        for (const auto &f : R.free) free_units += f.second;
        out[4 * k] = res; out[4 * k + 1] = (int64_t)R.end; out[4 * k + 2] = (int64_t)R.free.size(); out[4 * k + 3] = free_units;
    }
}

} // namespace ycge_host
