// The C++ mirror of the flip ensemble: dnn::tensorrt::set_flip_ensemble / flip_ensemble / batch_room and the stream's set_flip_ensemble.
//   flip_api.bin host   no device: the additions compile with plain g++; hp_flip_tables_coco gives involutions with -1 on the even PAF channels;
//                       hp_hflip_u8c3_host and hp_flip_merge_host agree with loops written here; the refusals return HP_ERR_INVALID.  Prints "HOST_OK".
//   flip_api.bin        on the GPU: with set_flip_ensemble(true), inference(frames) returns hp_flip_merge_host of the plain engine's maps on
//                       [frames, flipped frames], by memcmp, for network-sized frames (host batch) and frames that are resized (device batch);
//                       max_batch_size() / 2 + 1 frames and a float buffer throw std::logic_error; off again the maps are the plain ones.
//                       Prints "OK <comparisons>".
// Run by tests/test_cpp_flip.py.
#include <hyperpose/hyperpose.hpp>

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

namespace hp = hyperpose;

// compiled, never run on the host: the stream's switch sits next to set_orientation
[[maybe_unused]] static void stream_api(hp::dnn::tensorrt& engine, hp::parser::paf& parser)
{
    auto stream = hp::make_stream(engine, parser, true, false);
    stream.set_orientation(hp::orientation{});
    stream.set_flip_ensemble(true);
}

static int host_part()
{
    for (int cc : { 18, 19 }) {
        int32_t conf[19], perm[38];
        int8_t sign[38];
        if (hp_flip_tables_coco(cc, conf, perm, sign) != HP_OK)
            return 20;
        for (int c = 0; c < cc; ++c)
            if (conf[conf[c]] != c)
                return 21;
        for (int c = 0; c < 38; ++c)
            if (perm[perm[c]] != c || sign[c] != (c % 2 ? 1 : -1) || sign[perm[c]] != sign[c])
                return 22;
        if (conf[2] != 5 || conf[17] != 16 || conf[0] != 0 || perm[0] != 6 || perm[30] != 32)
            return 23;
    }
    int32_t conf[19], perm[38];
    int8_t sign[38];
    if (hp_flip_tables_coco(17, conf, perm, sign) != HP_ERR_INVALID)
        return 24;
    // the frame flip
    const int w = 5, h = 2, n = 2;
    std::vector<uint8_t> src((size_t)n * h * w * 3), dst(src.size(), 0);
    for (size_t i = 0; i < src.size(); ++i)
        src[i] = (uint8_t)(i * 37 + 11);
    if (hp_hflip_u8c3_host(src.data(), dst.data(), w, h, n) != HP_OK)
        return 25;
    for (int r = 0; r < n * h; ++r)
        for (int x = 0; x < w; ++x)
            for (int c = 0; c < 3; ++c)
                if (dst[((size_t)r * w + x) * 3 + c] != src[((size_t)r * w + (w - 1 - x)) * 3 + c])
                    return 26;
    if (hp_hflip_u8c3_host(src.data(), src.data() + 3, w, h, n) != HP_ERR_INVALID || hp_hflip_u8c3_host(src.data(), dst.data(), 0, h, n) != HP_ERR_INVALID)
        return 27;
    // the merge, one frame of 38 x 2 x 3 maps and a third map that must stay
    const int C = 38, H = 2, W = 3;
    std::vector<float> maps((size_t)3 * C * H * W);
    unsigned s = 3;
    for (auto& v : maps)
        s = s * 1664525u + 1013904223u, v = (float)(int)(s >> 16) / 4096.f - 8.f;
    std::vector<float> got = maps;
    if (hp_flip_merge_host(got.data(), 1, C, H, W, perm, sign) != HP_OK)
        return 28;
    for (int c = 0; c < C; ++c)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const float a = maps[((size_t)c * H + y) * W + x], b = maps[(((size_t)C + perm[c]) * H + y) * W + (W - 1 - x)];
                const float want = sign[c] < 0 ? 0.5f * (a - b) : 0.5f * (a + b);
                if (std::memcmp(&want, &got[((size_t)c * H + y) * W + x], sizeof want) != 0)
                    return 29;
            }
    if (std::memcmp(got.data() + (size_t)C * H * W, maps.data() + (size_t)C * H * W, sizeof(float) * 2 * C * H * W) != 0)
        return 30;
    sign[4] = 0;
    if (hp_flip_merge_host(got.data(), 1, C, H, W, perm, sign) != HP_ERR_INVALID)
        return 31;
    std::printf("HOST_OK\n");
    return 0;
}

static cv::Mat random_mat(int w, int h, unsigned seed)
{
    cv::Mat m(h, w);
    unsigned s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < (size_t)w * h * 3; ++i)
        s = s * 1664525u + 1013904223u, m.data()[i] = (uint8_t)(s >> 24);
    return m;
}

static size_t count_of(const hp::feature_map_t& m)
{
    size_t n = 1;
    for (int d : m.shape())
        n *= (size_t)d;
    return n;
}

// maps of [frames, flipped frames] from the plain engine -> what the ensemble must return for the frames
static std::vector<std::vector<float>> merged_by_hand(const std::vector<hp::internal_t>& plain, size_t n, size_t k)
{
    const auto shape = plain[0][k].shape(); // (C, H, W)
    const size_t one = count_of(plain[0][k]);
    std::vector<float> all(2 * n * one);
    for (size_t i = 0; i < 2 * n; ++i)
        std::memcpy(all.data() + i * one, plain[i][k].view<float>(), one * sizeof(float));
    int32_t conf[19], perm[38];
    int8_t sign[38], ones[19];
    std::fill(ones, ones + 19, (int8_t)1);
    if (hp_flip_tables_coco(k == 0 ? shape[0] : 19, conf, perm, sign) != HP_OK
        || hp_flip_merge_host(all.data(), (int)n, shape[0], shape[1], shape[2], k == 0 ? conf : perm, k == 0 ? ones : sign) != HP_OK)
        std::exit(3);
    std::vector<std::vector<float>> out;
    for (size_t i = 0; i < n; ++i)
        out.emplace_back(all.begin() + i * one, all.begin() + (i + 1) * one);
    return out;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::strcmp(argv[1], "host") == 0)
        return host_part();
    if (hp_init(0) != HP_OK) {
        std::printf("NO_DEVICE %s\n", hp_last_error());
        return 2;
    }
    int compared = 0;
    const int NW = 88, NH = 56;
    hp::dnn::tensorrt engine(hp::dnn::builtin_model{ "lw_openpose_vggtiny", {}, 7 }, cv::Size(NW, NH), 4, false);
    if (engine.flip_ensemble() || engine.batch_room() != 4)
        return 10;
    for (int sized = 0; sized < 2; ++sized) { // network-sized frames go up as one host batch, others are resized on the device
        const int w = sized ? NW : 150, h = sized ? NH : 100;
        // the flip is of the NETWORK-SIZED slot: for frames that are resized the reference runs on slots made by hand
        std::vector<cv::Mat> frames = { random_mat(w, h, 1 + sized), random_mat(w, h, 5 + sized) }, slots;
        for (const auto& f : frames) {
            cv::Mat slot(NH, NW);
            hp::detail::dev_ptr src((size_t)w * h * 3), dst((size_t)NW * NH * 3);
            if (hp_memcpy_h2d(src.p, f.data(), (size_t)w * h * 3) != HP_OK || hp_resize_u8c3((const uint8_t*)src.p, w, h, w * 3, (uint8_t*)dst.p, NW, NH, NW * 3, nullptr) != HP_OK
                || hp_device_synchronize() != HP_OK || hp_memcpy_d2h(slot.data(), dst.p, (size_t)NW * NH * 3) != HP_OK)
                return 11;
            slots.push_back(slot);
        }
        std::vector<cv::Mat> both = slots;
        for (const auto& sl : slots) {
            cv::Mat f(NH, NW);
            if (hp_hflip_u8c3_host(sl.data(), f.data(), NW, NH, 1) != HP_OK)
                return 12;
            both.push_back(f);
        }
        engine.set_flip_ensemble(false);
        const auto plain = engine.inference(both);
        const auto plain_frames = engine.inference(frames);
        engine.set_flip_ensemble(true);
        if (!engine.flip_ensemble() || engine.batch_room() != 2 || engine.max_batch_size() != 4)
            return 13;
        const auto got = engine.inference(frames);
        if (got.size() != 2 || got[0].size() != 2)
            return 14;
        for (size_t k = 0; k < 2; ++k) {
            const auto want = merged_by_hand(plain, 2, k);
            for (size_t i = 0; i < 2; ++i, ++compared)
                if (count_of(got[i][k]) != want[i].size() || std::memcmp(got[i][k].view<float>(), want[i].data(), want[i].size() * sizeof(float)) != 0)
                    return 15 + sized;
        }
        bool threw = false;
        try {
            engine.inference(std::vector<cv::Mat>{ frames[0], frames[1], frames[0] });
        } catch (const std::logic_error& e) {
            threw = std::strstr(e.what(), "Input batch size overflow") != nullptr && std::strstr(e.what(), "Max@2") != nullptr
                && std::strstr(e.what(), "max_batch_size 4 halved") != nullptr; // the message says why the room is not max_batch_size()
        }
        if (!threw)
            return 17;
        threw = false;
        try {
            engine.inference(std::vector<float>((size_t)3 * NW * NH), 1);
        } catch (const std::logic_error&) {
            threw = true;
        }
        if (!threw)
            return 18;
        engine.set_flip_ensemble(false); // off again: the plain maps
        const auto again = engine.inference(frames);
        for (size_t i = 0; i < 2; ++i)
            for (size_t k = 0; k < 2; ++k, ++compared)
                if (std::memcmp(again[i][k].view<float>(), plain_frames[i][k].view<float>(), count_of(again[i][k]) * sizeof(float)) != 0)
                    return 19;
    }
    // a network without the (conf, paf) pair is refused with the C ABI's message
    hp::dnn::tensorrt ppn(hp::dnn::builtin_model{ "pose_proposal_resnet50", {}, 3 }, cv::Size(96, 96), 2, false, hp::data_type::kHALF);
    bool threw = false;
    try {
        ppn.set_flip_ensemble(true);
    } catch (const std::logic_error& e) {
        threw = std::strstr(e.what(), "hp_engine_set_flip_ensemble_coco") != nullptr;
    }
    if (!threw || ppn.flip_ensemble())
        return 40;
    std::printf("OK %d\n", compared);
    return 0;
}
