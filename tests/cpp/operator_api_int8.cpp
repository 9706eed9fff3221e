// data_type::kINT8 through the mirror headers: a built-in model as a kINT8 engine, inference before calibrate() throws
// std::logic_error, calibrate + inference + parser::paf::process, save -> tensorrt_serialized gives the same maps, and make_stream
// works on the calibrated engine (and refuses an uncalibrated one).  Prints "OK <humans> <stream frames>"; run by
// tests/test_int8_cpu.py (compile) and tests/test_engine_int8_gpu.py (run).
#include <hyperpose/hyperpose.hpp>

#include <cstdio>
#include <cstring>
#include <stdexcept>

static std::vector<cv::Mat> frames(int n, int w, int h, int salt)
{
    std::vector<cv::Mat> v;
    for (int i = 0; i < n; ++i) {
        cv::Mat m(h, w);
        for (size_t k = 0; k < m.total() * 3; ++k)
            m.data()[k] = (uint8_t)((k * 31 + i * 7 + salt * 13 + (k / 97) * 5) & 255);
        v.push_back(m);
    }
    return v;
}

int main(int argc, char** argv)
{
    if (hp_init(0) != HP_OK) {
        std::printf("NO_DEVICE %s\n", hp_last_error());
        return 2;
    }
    namespace hp = hyperpose;
    const std::string saved = argc > 1 ? argv[1] : "operator_api_int8.hpeng";
    hp::dnn::tensorrt engine(hp::dnn::builtin_model{ "lw_openpose_vggtiny", {}, 7 }, cv::Size(64, 48), 3, false, hp::data_type::kINT8);
    const auto batch = frames(3, 64, 48, 1);
    bool threw = false;
    try {
        engine.inference(batch);
    } catch (const std::logic_error& e) {
        threw = std::strstr(e.what(), "calibrate()") != nullptr;
    }
    if (!threw)
        return 3;
    hp::parser::paf stream_parser{};
    bool stream_threw = false;
    try {
        auto s = hp::make_stream(engine, stream_parser);
    } catch (const std::logic_error& e) {
        stream_threw = std::strstr(e.what(), "calibrate()") != nullptr;
    }
    if (!stream_threw)
        return 4;
    engine.calibrate(frames(5, 80, 60, 2)); // any size, any count: resized like inference() does
    auto packets = engine.inference(batch);
    size_t humans = 0;
    hp::parser::paf parser(0.05f, -1e9f);
    for (auto& packet : packets)
        humans += parser.process(packet[0], packet[1]).size();
    engine.save(saved);
    hp::dnn::tensorrt back(hp::dnn::tensorrt_serialized{ saved }, cv::Size(64, 48), 3);
    auto again = back.inference(batch);
    for (size_t f = 0; f < packets.size(); ++f)
        for (size_t o = 0; o < packets[f].size(); ++o) {
            size_t n = 1;
            for (int d : packets[f][o].shape())
                n *= (size_t)d;
            if (std::memcmp(packets[f][o].view<float>(), again[f][o].view<float>(), n * sizeof(float)) != 0)
                return 5;
        }
    std::remove(saved.c_str());
    size_t stream_frames = 0;
    {
        auto stream = hp::make_stream(engine, stream_parser);
        std::vector<std::vector<hp::human_t>> out;
        auto in = frames(4, 64, 48, 3);
        stream.async() << in;
        stream.sync() >> out;
        stream_frames = out.size();
    }
    if (stream_frames != 4)
        return 6;
    std::printf("OK %zu %zu\n", humans, stream_frames);
    return 0;
}
