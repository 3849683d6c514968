// The image plan of one tf_fb_calc_slots call: which frame slots are expanded (A1+A2), in which runs of launches, and
// which two expansions every pair compares.  Pure host arithmetic over small integer arrays: nothing of HIP here, so a
// host compiler builds it alone (tools/fb_plan_host_check.cpp runs it under the sanitizers).
//
// A1+A2 depend on the frame alone, and consecutive pairs of a video share one: every slot the batch
// names is expanded once (16 consecutive pairs: 17 expansions, not 32) and each pair carries the
// indices of its two.  Option fb_no_share: one expansion per pair and side, as separate calls would do.
// With tf_fb_keep_expansions an image IS its slot and survives the call: only slots written since
// their last expansion are listed, in runs of consecutive slots (a run = one set of launches).
#pragma once

namespace tf {
namespace fb {

struct ImagePair { // the two expansions of a pair; laid out as the int2 the kernels read
    int x, y;
};

struct ImageRun {
    int image0, list0, n; // first image index written, offset into the image list (even), images
};

// The caller's storage.  The kernels read the list two entries at a time (int2), so every run starts at an even offset
// and is padded to an even length with its first slot.
struct ImagePlan {
    int *image_of;   // [slots] scratch: slot -> index in the list (share), needed or not (keep)
    int *list;       // the slots to expand, run after run
    int list_cap;
    ImagePair *map;  // [n_pairs] pair -> its two images
    ImageRun *runs;
    int run_cap;
    int n_list, n_runs; // written
};

// prev_slots, next_slots: [n_pairs], every entry in [0, slots).  expanded, external: [slots], read with `keep` only: the
// expansion is valid / the slot is written behind the library's back.
// false: the list or the runs do not fit the storage (nothing past it is written)
inline bool plan_images(ImagePlan &out, int slots, int n_pairs, const int *prev_slots, const int *next_slots, bool keep,
                        bool no_share, const char *expanded, const char *external)
{
    int n = 0;
    out.n_list = out.n_runs = 0;
    auto put = [&](int slot) {
        if (n >= out.list_cap)
            return false;
        out.list[n++] = slot;
        return true;
    };
    for (int s = 0; s < slots; s++)
        out.image_of[s] = -1;
    if (keep) {
        for (int i = 0; i < n_pairs; i++) {
            const int sl[2] = {prev_slots[i], next_slots[i]};
            for (int s : sl)
                if (!expanded[s] || external[s])
                    out.image_of[s] = 1;
            out.map[i] = ImagePair{prev_slots[i], next_slots[i]};
        }
        for (int s = 0; s < slots;) { // in slot order: a run ends at the first slot that is not needed
            if (out.image_of[s] < 0) {
                s++;
                continue;
            }
            if (out.n_runs >= out.run_cap)
                return false;
            const int first = s, off = n;
            for (; s < slots && out.image_of[s] >= 0; s++)
                if (!put(s))
                    return false;
            if ((n & 1) && !put(first))
                return false;
            out.runs[out.n_runs++] = ImageRun{first, off, s - first};
        }
    } else {
        if (out.run_cap < 1)
            return false;
        for (int i = 0; i < n_pairs; i++) {
            int im[2];
            const int sl[2] = {prev_slots[i], next_slots[i]};
            for (int j = 0; j < 2; j++) {
                if (no_share || out.image_of[sl[j]] < 0) { // first seen: the next image
                    out.image_of[sl[j]] = n;
                    if (!put(sl[j]))
                        return false;
                }
                im[j] = out.image_of[sl[j]];
            }
            out.map[i] = ImagePair{im[0], im[1]};
        }
        const int n_images = n;
        if ((n & 1) && !put(out.list[0])) // the unused half of the last int2
            return false;
        out.runs[out.n_runs++] = ImageRun{0, 0, n_images};
    }
    out.n_list = n;
    return true;
}

} // namespace fb
} // namespace tf
