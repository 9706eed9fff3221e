// What the three parser mirrors (paf.hpp, proposal_network.hpp, pifpaf.hpp) share: the whole-batch cache, the hp_human -> human_t
// conversion and the reference's error() (print + std::exit(-1), src/logging.hpp:31-37).
#pragma once
#include <cstdlib>
#include <iostream>
#include <memory>
#include <vector>

#include "../../../hp_hip.h"
#include "../../utility/data.hpp"

namespace hyperpose {
namespace detail {

    // (paf prints the message as it is, the other two end the line)
    [[noreturn]] inline void fatal(const char* msg, bool newline)
    {
        std::cerr << "[HyperPose::ERROR  ] " << msg;
        if (newline)
            std::cerr << "\n";
        std::exit(-1);
    }

    inline std::vector<human_t> to_humans(const hp_human* out, int n)
    {
        std::vector<human_t> ret(n);
        for (int i = 0; i < n; ++i) {
            ret[i].score = out[i].score;
            for (int k = 0; k < COCO_N_PARTS; ++k)
                ret[i].parts[k] = body_part_t{ out[i].parts[k].has_value != 0, out[i].parts[k].x, out[i].parts[k].y, out[i].parts[k].score };
        }
        return ret;
    }
    // n frames through process_batch(out, cap, n_out) - a parser's hp_*_process_batch with room for 128 humans per frame - or fatal()
    template <typename Call>
    std::vector<std::vector<human_t>> parse_batch(int n, bool newline, Call&& process_batch)
    {
        constexpr int CAP = 128;
        std::vector<hp_human> out((size_t)n * CAP);
        std::vector<int> cnt(n);
        if (process_batch(out.data(), CAP, cnt.data()) != HP_OK)
            fatal(hp_last_error(), newline);
        std::vector<std::vector<human_t>> res(n);
        for (int f = 0; f < n; ++f)
            res[f] = to_humans(out.data() + (size_t)f * CAP, cnt[f]);
        return res;
    }

    // Maps that still lie in their engine's device buffers (utility/data.hpp, device_batch) are read from there - no D2H + H2D round trip -
    // and, because the reference's callers ask for the frames of a batch one after the other
    // (examples/operator_api_batched_images_paf.example.cpp:70-73), the WHOLE batch is parsed in one launch the first time one of its frames
    // is asked for; the other frames' calls return what that launch found.  Per frame the result is process()'s own: the kernels are the
    // same and frames are independent (tests/cpp/operator_api_paf.cpp compares the two paths).
    class batch_cache {
    public:
        // The humans of first_map's frame, or null when the maps have to take the per-frame path: no device batch behind them (any more),
        // HP_MIRROR_HOST_MAPS set, or !same_batch - the parser's own test that all its maps are the same frame of that batch (and whatever
        // else its policy asks).  parse_whole_batch(batch) -> one list per frame.
        template <typename Parse>
        const std::vector<human_t>* frame(const feature_map_t& first_map, bool same_batch, Parse&& parse_whole_batch)
        {
            const device_batch* b = first_map.device_batch();
            if (!b || !same_batch || std::getenv("HP_MIRROR_HOST_MAPS"))
                return nullptr;
            if (m_batch.lock().get() != b || m_gen != b->gen) {
                m_lists = parse_whole_batch(*b);
                m_batch = first_map.batch_handle(), m_gen = b->gen;
            }
            return &m_lists[first_map.batch_frame()];
        }
        void reset() { m_batch.reset(); } // a setter changed what a parse would find

    private:
        std::weak_ptr<device_batch> m_batch; // the batch m_lists holds the humans of
        uint64_t m_gen = 0;
        std::vector<std::vector<human_t>> m_lists;
    };

} // namespace detail
} // namespace hyperpose
