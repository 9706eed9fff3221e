// hyperpose::parser::pifpaf over libhp_hip.so — reference include/hyperpose/operator/parser/pifpaf.hpp:8-26.
// process(arg0, arg1): arg0 = PAF/CAF [19,9,h,w], arg1 = PIF/CIF [17,5,h,w] (the reference's .cpp parameter order,
// src/pifpaf.cpp:7; its header names them the other way round).  The engine also emits them as [171,h,w] / [85,h,w].
#pragma once
#include <cassert>

#include "detail.hpp"

namespace hyperpose::parser {

class pifpaf {
public:
    inline explicit pifpaf(int h, int w, float thresh = 0.1)
        : m_net_h(h), m_net_w(w), m_keypoint_thresh(thresh) {}
    pifpaf(const pifpaf& p)
        : m_net_h(p.m_net_h), m_net_w(p.m_net_w), m_keypoint_thresh(p.m_keypoint_thresh) {}
    ~pifpaf() { hp_pifpaf_destroy(m_h); }
    hp_parser_desc stream_desc() const
    {
        hp_parser_desc d{};
        d.kind = HP_PARSER_PIFPAF;
        d.thresh[0] = m_keypoint_thresh;
        d.res_w = d.res_h = -1;
        return d;
    }

    std::vector<human_t> process(const feature_map_t& paf, const feature_map_t& pif)
    {
        const int fh = pif.shape()[pif.shape().size() - 2], fw = pif.shape().back(); // src/pifpaf.cpp:23-24
        // maps that still lie in their engine's device buffers: the whole batch in one launch (detail.hpp, batch_cache)
        const bool same = paf.device_batch() == pif.device_batch() && paf.batch_frame() == pif.batch_frame();
        if (const std::vector<human_t>* hit = m_cache.frame(paf, same, [&](const detail::device_batch& b) {
                return run(b.n, b.outs[paf.batch_output()].dev, b.outs[pif.batch_output()].dev, fh, fw, 1);
            }))
            return *hit;
        return std::move(run(1, paf.view<float>(), pif.view<float>(), fh, fw, 0)[0]);
    }
    template <typename C>
    std::vector<human_t> process(C&& feature_map_containers)
    {
        assert(feature_map_containers.size() == 2);
        return process(feature_map_containers[0], feature_map_containers[1]);
    }

private:
    [[noreturn]] static void fatal(const char* msg) { detail::fatal(msg, true); }
    std::vector<std::vector<human_t>> run(int n, const float* paf, const float* pif, int fh, int fw, int on_device)
    {
        ensure(n);
        return detail::parse_batch(n, true, [&](hp_human* out, int cap, int* cnt) { return hp_pifpaf_process_batch(m_h, n, paf, pif, fh, fw, on_device, out, cap, cnt); });
    }
    void ensure(int batch) // a decoder handle that takes `batch` frames per call (rebuilt when a larger batch arrives)
    {
        if (m_h && batch <= m_handle_batch)
            return;
        hp_pifpaf_destroy(m_h);
        m_h = nullptr;
        if (hp_pifpaf_create(&m_h, m_net_h, m_net_w, m_keypoint_thresh, batch) != HP_OK)
            fatal(hp_last_error());
        m_handle_batch = batch;
    }
    int m_net_h, m_net_w;
    float m_keypoint_thresh;
    hp_pifpaf* m_h = nullptr;
    int m_handle_batch = 0;
    detail::batch_cache m_cache;
};

} // namespace hyperpose::parser
