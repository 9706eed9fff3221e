// examples/cli.cpp — `hyperpose-cli` on the MI355X engine.  What is kept from the reference's examples/cli.cpp is its INTERFACE: the flag
// names and defaults (:15-35: model / post / w / h / max_batch_size / source / runtime / keep_ratio / alpha / saving_prefix / logging /
// imshow), the values `operator` / `stream` and `paf` / `ppn` / `pifpaf`, the model-file suffix rule (.onnx / .uff / anything else =
// serialized engine) and the order of the work (resize + inference, parse, resume_ratio, draw, blend with weight alpha, write).  The
// program itself is written for this engine; the pieces that need gflags and OpenCV are replaced by what this image has:
//   * flags: `--name=value`, `--name value`, `--flag` / `--noflag` (gflags syntax), parsed below;
//   * media: binary PPM (P6) images - one file, or every *.ppm of a directory - and `synthetic:<n>:<w>x<h>` (seeded frames); results are
//     written as `<saving_prefix>_<id>.ppm` with the skeletons drawn (hp::draw_human) and blended with weight alpha.  With OpenCV
//     (-DHYPERPOSE_USE_OPENCV) any cv::imread format works; videos / the camera need cv::VideoCapture and are refused without it.
//   * video frames (addition): `--source=<file>.yuv` reads raw video (e.g. `ffmpeg -pix_fmt yuv420p -f rawvideo`) frames of
//     `--yuv_w` x `--yuv_h` in the layout `--yuv_format=i420|nv12|p010|i010|nv16|i422|yuy2|uyvy|i444` (default i420), colours
//     `--yuv_matrix=bt601|bt709|bt2020` and `--yuv_range=limited|full` (defaults bt601, limited); `--yuv` converts any other source to
//     NV12 first.  Either way the operator runtime hands the engine hyperpose::yuv_frame batches (colour conversion fused into the resize
//     on the GPU); the BGR pictures, converted on the host with the same table (hp_yuv_coefficients), are only drawn on.
//   * packed RGB / grey frames (addition): `--rgb=<rgb24|bgr24|bgra|rgba|argb|abgr|gray>` feeds every frame of any source to the engine as an
//     hyperpose::rgb_frame of that layout (hp_rgb_image: read by the fused resize, nothing is repacked for the engine).  The frame is made on the host
//     from the BGR picture: alpha 255, grey = (B + 2 G + R + 2) >> 2.  `--source=<file>.rgb` reads raw frames of `--yuv_w` x `--yuv_h` in that layout,
//     back to back.  Operator runtime (as --yuv); refused from the flags alone: an unknown name, --rgb with --yuv or a .yuv source, --saving_yuv or
//     --redact with --rgb (drawing and redaction have no RGB targets; --redact is allowed where --encode_yuv makes the target), a .rgb source
//     without --rgb.
//   * HDR video (addition): `--yuv_transfer=sdr|pq|hlg` (default sdr) `[--hdr_peak=<cd/m2> --hdr_white=<cd/m2> --hdr_keep_primaries]`, only with
//     a .yuv source in a 10-bit layout (`--yuv_format=p010|i010`): the frames are HDR10 (pq) or HLG and are tone-mapped to SDR sRGB inside the
//     fused resize (engine.set_tonemap; hp::hdr, defaults 1000 / 203, BT.2020 primaries converted to BT.709 unless --hdr_keep_primaries); the
//     pictures drawn on are converted on the host by the same rule (hp_tonemap_convert_host), and with --saving_yuv the skeletons are drawn with
//     the HDR colours (graphics white at --hdr_white);
//   * tiled inference (addition): `--tiles=<columns>x<rows> [--tile_overlap=<px>] [--tile_full]`: every frame - BGR or --yuv / .yuv, with or
//     without --saving_yuv - is inferred on overlapping tiles (one engine call per frame, engine.inference(frame, regions)) and the humans
//     are merged in the frame's coordinates (hp::plan_tiles / to_frame / merge_humans; stream runtime: stream.set_tiling);
//   * flip ensemble (addition): `--flip_ensemble`: every frame - every tile of it with --tiles - runs through the network with its left-right
//     flip and the parser reads the merged maps (engine.set_flip_ensemble / stream.set_flip_ensemble; include/hp_hip.h "flip ensemble"); a batch
//     then holds --max_batch_size / 2 frames.  --post=paf only; works in both runtimes and with --tiles, --rotate, --hflip and --yuv_*;
//   * scale ensemble (addition): `--scale_ensemble=<s>[,<s>...]` (1 .. 3 scales in (0, 1], e.g. 0.5,0.75): every frame - every tile of it - also runs
//     shrunk by each scale and the parser reads the maps averaged over the K = count + 1 passes (engine.set_scale_ensemble /
//     stream.set_scale_ensemble; include/hp_hip.h "scale ensemble"); a batch then holds --max_batch_size / K frames (/ 2K with --flip_ensemble).
//     --post=paf only; both runtimes;
//   * upright input (addition): `--rotate=0|90|180|270` (the clockwise turn that brings the stored picture upright: a container's rotate tag) and
//     `--hflip` (the stored picture is mirrored left-right): the frames of every source, in both runtimes, are read upright inside the resize
//     (engine.set_orientation / stream.set_orientation; hp::orientation).  Pictures and --saving_yuv frames stay in stored orientation, the
//     skeletons are drawn through hp::to_stored; <file>.humans holds the upright records.  Tiles are planned on the upright frame;
//   * writing video back (addition): `--saving_yuv=<file>`, for a .yuv source or `--yuv`: every frame is uploaded in its own format, inference
//     runs on it as a device-resident frame, the skeletons are drawn on the device surface (hp::draw_humans, opacity = alpha; alpha == 0 -> 1)
//     and the annotated frames are appended to <file> as raw frames of the same format; <file>.humans receives, per frame, an int32 count and
//     that many 292-byte hp_human records in the frame's coordinates (what was drawn).  The PPM output is unchanged.
//   * map view (addition): `--show_maps=conf|paf` blends the network's own maps - the largest confidence channel, or the longest part-affinity
//     vector - into the --saving_yuv frames on the device surface (hp::draw_maps: `--maps_palette=jet|heat|grey`, `--maps_alpha=constant|scaled`,
//     `--maps_opacity=0.5`, `--maps_gain=1`), AFTER the redaction and BEFORE the skeletons.  Operator runtime, --post=paf, no --tiles; refused
//     from the flags alone without --saving_yuv, with --runtime=stream or with a bad value.
//   * redaction (addition): `--redact=head|body` pixelates (`--redact_effect=pixelate|black`) the heads or the whole persons on the --saving_yuv
//     frames, on the device surface (hp::redact_humans: cells of `--redact_cell=16` pixels, regions grown by `--redact_margin=1.0`), BEFORE the
//     skeletons are drawn on top; `--redact_only` leaves the skeletons out.  Refused from the flags alone without --saving_yuv or with a bad value.
//   * encoder hand-off (addition): `--encode_yuv=<file> [--encode_format=nv12 --encode_matrix=bt709 --encode_range=limited --encode_align=2]`, for
//     picture sources and `--rgb=<layout>` / .rgb sources: every frame is uploaded in its own layout (BGR24 pictures, or the --rgb layout),
//     converted on the device to the frame an encoder takes (hp::to_yuv: any --yuv_format name, the stream's matrix and range, the size rounded up to
//     --encode_align and to what the layout needs, by edge replication), `--redact` and the skeletons are applied on that surface as --saving_yuv
//     applies them, and the frame is appended to <file>; <file>.humans is written as --saving_yuv writes it (the records are normalised to the
//     source frame, without the padding).  Operator runtime.  Refused from the flags alone: with --yuv or a .yuv source (those have --saving_yuv),
//     an unknown name, --encode_align outside 1 .. 256, the companions without --encode_yuv.
//   * `--synthetic_humans=<n>` (addition, default 0): n seeded stand-in humans are added to every frame's parser output before anything is drawn -
//     the built-in models carry synthetic weights and find nobody, so this is what makes a demonstration (or a test) of the drawing paths show
//     something; operator runtime only.  A warning says that the pictures and the count are not the model's result.
//   * `--model`: .onnx, a serialized engine (anything else), or `builtin:<arch>` (hp_model_archs(); synthetic weights).
// build: g++ -std=c++17 -O2 -Iinclude examples/cli.cpp -Lhyperpose_amd -lhp_hip -lpthread -Wl,-rpath,$PWD/hyperpose_amd -o hyperpose-cli
#include <hyperpose/hyperpose.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <dirent.h>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <string_view>
#include <variant>

#define kOPERATOR "operator"
#define kSTREAM "stream"
#define kPAF "paf"
#define kPPN "ppn"
#define kPIFPAF "pifpaf"

namespace hp = hyperpose;

// ---- flags (defaults of examples/cli.cpp:15-35)
static std::string FLAGS_model = "builtin:lw_openpose_mobilenet";
static std::string FLAGS_post = kPAF;
static int FLAGS_w = 368, FLAGS_h = 342, FLAGS_max_batch_size = 6;
static bool FLAGS_imshow = true;
static std::string FLAGS_source = "synthetic:4:640x480";
static std::string FLAGS_runtime = kOPERATOR;
static bool FLAGS_keep_ratio = true;
static double FLAGS_alpha = 0.5;
static std::string FLAGS_saving_prefix = "output";
static bool FLAGS_logging = false;
static bool FLAGS_half = false; // addition: data_type::kHALF engines (the reference CLI always builds data_type::kFLOAT ones)
static bool FLAGS_int8 = false; // addition: data_type::kINT8 engines, calibrated on the first batch of the source
static bool FLAGS_yuv = false;  // addition: feed the engine video frames (dnn::tensorrt::inference(std::vector<yuv_frame>)); implied by a .yuv source
static int FLAGS_yuv_w = 0, FLAGS_yuv_h = 0; // frame size of a raw .yuv source
static std::string FLAGS_yuv_format = "i420", FLAGS_yuv_matrix = "bt601", FLAGS_yuv_range = "limited"; // layout and colours of a raw .yuv source
static std::string FLAGS_yuv_transfer = "sdr"; // addition: pq | hlg: the 10-bit frames of a .yuv source are HDR10 / HLG (hp::hdr)
static double FLAGS_hdr_peak = HP_HDR_DEFAULT_PEAK, FLAGS_hdr_white = HP_HDR_DEFAULT_WHITE; // ... the tone curve's parameters, cd/m2
static bool FLAGS_hdr_keep_primaries = false;  // ... leave the BT.2020 primaries as they are
static bool g_hdr_on = false;
static hp::hdr g_hdr;
static std::string FLAGS_tiles;      // addition: --tiles CxR: inference on C x R overlapping tiles of every frame, the humans merged (hp::tiling)
static int FLAGS_tile_overlap = 64;  // ... pixels neighbouring tiles share at least
static bool FLAGS_tile_full = false; // ... plus the whole frame as one more region
static bool g_tiled = false;
static hp::tiling g_tiling;
static int FLAGS_rotate = 0;       // addition: --rotate=0|90|180|270: clockwise degrees that bring the stored frames upright (hp::orientation)
static bool FLAGS_hflip = false;   // ... the stored frames are mirrored left-right
static bool FLAGS_flip_ensemble = false; // addition: --flip_ensemble: frame + flipped frame through the network, maps merged on the device (PAF only)
static std::string FLAGS_scale_ensemble; // addition: --scale_ensemble=0.5,0.75: frame + shrunken frames through the network, maps merged (PAF only)
static std::vector<float> g_scales;      // ... parsed
static hp::orientation g_orient;
static std::string FLAGS_saving_yuv; // addition: append the frames, annotated on the device in their own format, to this file
static std::string FLAGS_redact, FLAGS_redact_effect = "pixelate"; // addition: --redact=head|body on the --saving_yuv frames (hp::redaction)
static int FLAGS_redact_cell = 16;
static double FLAGS_redact_margin = 1.0;
static bool FLAGS_redact_only = false; // ... and no skeletons on top
static bool g_redact = false;
static std::string FLAGS_rgb; // addition: --rgb=<layout>: feed the engine packed RGB / grey frames (dnn::tensorrt::inference(std::vector<rgb_frame>))
static int g_rgb_format = -1; // ... parsed: HP_RGB_*, -1 while off
static hp::redaction g_redaction;
static std::string FLAGS_show_maps, FLAGS_maps_palette = "jet", FLAGS_maps_alpha = "constant"; // addition: --show_maps=conf|paf on the --saving_yuv frames (hp::map_view)
static double FLAGS_maps_opacity = 0.5, FLAGS_maps_gain = 1.0;
static bool g_show_maps = false;
static hp::map_view g_map_view;
static std::string FLAGS_encode_yuv, FLAGS_encode_format = "nv12", FLAGS_encode_matrix = "bt709", FLAGS_encode_range = "limited"; // addition: --encode_yuv=<file> (hp::to_yuv)
static int FLAGS_encode_align = 2;
static int g_encode_format = HP_YUV_NV12, g_encode_matrix = HP_YUV_BT709, g_encode_range = HP_YUV_LIMITED; // ... parsed
static int FLAGS_synthetic_humans = 0; // addition: stand-in humans added to every frame's poses (see the head of the file)
static bool g_yuv_from_file = false; // the frames came from a .yuv source (else --yuv made NV12 ones)
static int g_yuv_format = HP_YUV_I420, g_yuv_matrix = HP_YUV_BT601, g_yuv_range = HP_YUV_LIMITED;      // the same, parsed

static const char* FLAGS_yuv_format_written() { return g_yuv_from_file ? FLAGS_yuv_format.c_str() : "nv12"; }
static std::ostream& cli_log() { return std::cout << "[HyperPose::CLI] "; }

static bool parse_flags(int argc, char** argv)
{
    std::map<std::string, std::string*> sflags = { { "model", &FLAGS_model }, { "post", &FLAGS_post }, { "source", &FLAGS_source },
        { "runtime", &FLAGS_runtime }, { "saving_prefix", &FLAGS_saving_prefix }, { "saving_yuv", &FLAGS_saving_yuv }, { "tiles", &FLAGS_tiles }, { "yuv_format", &FLAGS_yuv_format },
        { "yuv_matrix", &FLAGS_yuv_matrix }, { "yuv_range", &FLAGS_yuv_range }, { "yuv_transfer", &FLAGS_yuv_transfer },
        { "scale_ensemble", &FLAGS_scale_ensemble }, { "redact", &FLAGS_redact }, { "redact_effect", &FLAGS_redact_effect }, { "rgb", &FLAGS_rgb },
        { "show_maps", &FLAGS_show_maps }, { "maps_palette", &FLAGS_maps_palette }, { "maps_alpha", &FLAGS_maps_alpha },
        { "encode_yuv", &FLAGS_encode_yuv }, { "encode_format", &FLAGS_encode_format }, { "encode_matrix", &FLAGS_encode_matrix }, { "encode_range", &FLAGS_encode_range } };
    std::map<std::string, double*> dflags = { { "alpha", &FLAGS_alpha }, { "hdr_peak", &FLAGS_hdr_peak }, { "hdr_white", &FLAGS_hdr_white },
        { "redact_margin", &FLAGS_redact_margin }, { "maps_opacity", &FLAGS_maps_opacity }, { "maps_gain", &FLAGS_maps_gain } };
    std::map<std::string, int*> iflags = { { "w", &FLAGS_w }, { "h", &FLAGS_h }, { "max_batch_size", &FLAGS_max_batch_size }, { "tile_overlap", &FLAGS_tile_overlap },
        { "yuv_w", &FLAGS_yuv_w }, { "yuv_h", &FLAGS_yuv_h }, { "synthetic_humans", &FLAGS_synthetic_humans }, { "rotate", &FLAGS_rotate },
        { "redact_cell", &FLAGS_redact_cell }, { "encode_align", &FLAGS_encode_align } };
    std::map<std::string, bool*> bflags = { { "imshow", &FLAGS_imshow }, { "keep_ratio", &FLAGS_keep_ratio }, { "logging", &FLAGS_logging }, { "half", &FLAGS_half }, { "int8", &FLAGS_int8 }, { "yuv", &FLAGS_yuv }, { "tile_full", &FLAGS_tile_full },
        { "hdr_keep_primaries", &FLAGS_hdr_keep_primaries }, { "hflip", &FLAGS_hflip }, { "flip_ensemble", &FLAGS_flip_ensemble },
        { "redact_only", &FLAGS_redact_only } };
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (a.rfind("--", 0) != 0 && a.rfind("-", 0) == 0)
            a = "-" + a; // gflags accepts -flag too
        if (a.rfind("--", 0) != 0) {
            cli_log() << "ERROR: unexpected argument " << a << "\n";
            return false;
        }
        a = a.substr(2);
        std::string name = a, value;
        bool has_value = false;
        if (const auto eq = a.find('='); eq != std::string::npos)
            name = a.substr(0, eq), value = a.substr(eq + 1), has_value = true;
        if (bflags.count(name) || (name.rfind("no", 0) == 0 && bflags.count(name.substr(2)))) {
            const bool neg = !bflags.count(name);
            bool v = !neg;
            if (has_value)
                v = (value == "true" || value == "1" || value == "yes") != neg;
            *bflags[neg ? name.substr(2) : name] = v;
            continue;
        }
        if (!has_value) {
            if (i + 1 >= argc) {
                cli_log() << "ERROR: flag --" << name << " needs a value\n";
                return false;
            }
            value = argv[++i];
        }
        if (sflags.count(name))
            *sflags[name] = value;
        else if (name == "rotate") { // an enumerated number: anything else, "90deg" or an empty value included, is refused with the list
            char* end = nullptr;
            const long v = std::strtol(value.c_str(), &end, 10);
            if (value.empty() || *end || (v != 0 && v != 90 && v != 180 && v != 270)) {
                cli_log() << "ERROR: --rotate=" << value << " is not one of 0|90|180|270 (clockwise degrees that bring the stored picture upright)\n";
                return false;
            }
            FLAGS_rotate = (int)v;
        } else if (iflags.count(name))
            *iflags[name] = std::atoi(value.c_str());
        else if (dflags.count(name))
            *dflags[name] = std::atof(value.c_str());
        else {
            cli_log() << "ERROR: unknown command line flag '" << name << "'\n";
            return false;
        }
    }
    g_orient = hp::orientation{ FLAGS_rotate / 90, FLAGS_hflip };
    if (!FLAGS_tiles.empty()) { // --tiles CxR, both counts >= 1
        int c = 0, r = 0;
        char x = 0, rest = 0;
        if (std::sscanf(FLAGS_tiles.c_str(), "%d%c%d%c", &c, &x, &r, &rest) != 3 || (x != 'x' && x != 'X') || c < 1 || r < 1 || c * r + (FLAGS_tile_full ? 1 : 0) > 64
            || FLAGS_tile_overlap < 0) {
            cli_log() << "ERROR: --tiles=" << FLAGS_tiles << " --tile_overlap=" << FLAGS_tile_overlap
                      << ": expected --tiles=<columns>x<rows> with both counts >= 1, at most 64 regions, and an overlap >= 0\n";
            return false;
        }
        g_tiled = true;
        g_tiling.cols = c, g_tiling.rows = r, g_tiling.overlap_x = g_tiling.overlap_y = FLAGS_tile_overlap, g_tiling.with_full = FLAGS_tile_full;
    } else if (FLAGS_tile_full) {
        cli_log() << "ERROR: --tile_full adds the whole frame to the tiles of --tiles=<columns>x<rows>\n";
        return false;
    }
    // the three enumerated flags: a value outside the list is refused with the list
    auto pick = [](const char* flag, const std::string& value, const std::vector<std::pair<const char*, int>>& names, int& out) {
        std::string all;
        for (const auto& [name, code] : names) {
            if (value == name) {
                out = code;
                return true;
            }
            all += (all.empty() ? "" : "|") + std::string(name);
        }
        cli_log() << "ERROR: --" << flag << "=" << value << " is not one of " << all << "\n";
        return false;
    };
    int transfer = 0;
    if (!pick("yuv_transfer", FLAGS_yuv_transfer, { { "sdr", 0 }, { "pq", HP_TRC_PQ }, { "hlg", HP_TRC_HLG } }, transfer))
        return false;
    if (transfer != 0) { // HDR: a 10-bit .yuv source, and a description the library accepts (its message names what is wrong)
        const bool from_file = FLAGS_source.size() >= 4 && FLAGS_source.compare(FLAGS_source.size() - 4, 4, ".yuv") == 0;
        if (!from_file || (FLAGS_yuv_format != "p010" && FLAGS_yuv_format != "i010")) {
            cli_log() << "ERROR: --yuv_transfer=" << FLAGS_yuv_transfer << " needs a .yuv source in a 10-bit layout (--yuv_format=p010|i010), got --yuv_format="
                      << FLAGS_yuv_format << (from_file ? "" : " and no .yuv source") << "\n";
            return false;
        }
        g_hdr.transfer = transfer, g_hdr.to_bt709 = !FLAGS_hdr_keep_primaries, g_hdr.peak_nits = (float)FLAGS_hdr_peak, g_hdr.white_nits = (float)FLAGS_hdr_white;
        const hp_hdr_desc d = g_hdr.c_form();
        std::vector<uint16_t> lin(1024);
        std::vector<uint8_t> out(4096);
        int32_t m[9];
        if (hp_tonemap_tables(&d, lin.data(), m, out.data()) != HP_OK) {
            cli_log() << "ERROR: --hdr_peak=" << FLAGS_hdr_peak << " --hdr_white=" << FLAGS_hdr_white << ": " << hp_last_error() << "\n";
            return false;
        }
        g_hdr_on = true;
    } else if (FLAGS_hdr_keep_primaries || FLAGS_hdr_peak != HP_HDR_DEFAULT_PEAK || FLAGS_hdr_white != HP_HDR_DEFAULT_WHITE) {
        cli_log() << "ERROR: --hdr_peak / --hdr_white / --hdr_keep_primaries describe the frames of --yuv_transfer=pq|hlg\n";
        return false;
    }
    // --rgb: an enumerated layout; what it cannot go with is settled here, from the flags alone
    const bool rgb_file = FLAGS_source.size() >= 4 && FLAGS_source.compare(FLAGS_source.size() - 4, 4, ".rgb") == 0;
    if (!FLAGS_rgb.empty()) {
        if (!pick("rgb", FLAGS_rgb, { { "rgb24", HP_RGB_RGB24 }, { "bgr24", HP_RGB_BGR24 }, { "bgra", HP_RGB_BGRA32 }, { "rgba", HP_RGB_RGBA32 }, { "argb", HP_RGB_ARGB32 },
                                       { "abgr", HP_RGB_ABGR32 }, { "gray", HP_RGB_GRAY8 } }, g_rgb_format))
            return false;
        const bool yuv_file = FLAGS_source.size() >= 4 && FLAGS_source.compare(FLAGS_source.size() - 4, 4, ".yuv") == 0;
        if (FLAGS_yuv || yuv_file) {
            cli_log() << "ERROR: --rgb=" << FLAGS_rgb << " and --yuv (or a .yuv source) both say how the engine is fed: give one\n";
            return false;
        }
        if (!FLAGS_saving_yuv.empty() || (!FLAGS_redact.empty() && FLAGS_encode_yuv.empty())) { // (--encode_yuv makes the frames --redact rewrites)
            cli_log() << "ERROR: --saving_yuv and --redact write video frames; with --rgb=" << FLAGS_rgb << " there is none (drawing and redaction have no RGB targets)\n";
            return false;
        }
    } else if (rgb_file) {
        cli_log() << "ERROR: a .rgb source holds raw frames: say their layout with --rgb=<rgb24|bgr24|bgra|rgba|argb|abgr|gray> (and --yuv_w, --yuv_h)\n";
        return false;
    }
    // --encode_yuv and its companions: enumerated names, an alignment in [1, 256], a source that is not video already
    if (!FLAGS_encode_yuv.empty()) {
        const bool yuv_file = FLAGS_source.size() >= 4 && FLAGS_source.compare(FLAGS_source.size() - 4, 4, ".yuv") == 0;
        if (FLAGS_yuv || yuv_file) {
            cli_log() << "ERROR: --encode_yuv converts pictures and --rgb frames to video frames; --yuv and .yuv sources are video already: write them with --saving_yuv=<file>\n";
            return false;
        }
        if (!pick("encode_format", FLAGS_encode_format, { { "i420", HP_YUV_I420 }, { "nv12", HP_YUV_NV12 }, { "p010", HP_YUV_P010 }, { "i010", HP_YUV_I010 },
                                                            { "nv16", HP_YUV_NV16 }, { "i422", HP_YUV_I422 }, { "yuy2", HP_YUV_YUY2 }, { "uyvy", HP_YUV_UYVY }, { "i444", HP_YUV_I444 } }, g_encode_format)
            || !pick("encode_matrix", FLAGS_encode_matrix, { { "bt601", HP_YUV_BT601 }, { "bt709", HP_YUV_BT709 }, { "bt2020", HP_YUV_BT2020 } }, g_encode_matrix)
            || !pick("encode_range", FLAGS_encode_range, { { "limited", HP_YUV_LIMITED }, { "full", HP_YUV_FULL } }, g_encode_range))
            return false;
        if (FLAGS_encode_align < 1 || FLAGS_encode_align > 256) {
            cli_log() << "ERROR: --encode_align=" << FLAGS_encode_align << " is outside [1, 256]\n";
            return false;
        }
    } else if (FLAGS_encode_format != "nv12" || FLAGS_encode_matrix != "bt709" || FLAGS_encode_range != "limited" || FLAGS_encode_align != 2) {
        cli_log() << "ERROR: --encode_format / --encode_matrix / --encode_range / --encode_align describe --encode_yuv=<file>\n";
        return false;
    }
    // --redact and its companions: enumerated names, an even cell in [2, 128], a margin in (0, 8]; the companions describe --redact
    if (!FLAGS_redact.empty()) {
        if (!pick("redact", FLAGS_redact, { { "head", hp::redaction::head }, { "body", hp::redaction::body } }, g_redaction.what)
            || !pick("redact_effect", FLAGS_redact_effect, { { "pixelate", hp::redaction::pixelate }, { "black", hp::redaction::black } }, g_redaction.effect))
            return false;
        if (FLAGS_redact_cell < 2 || FLAGS_redact_cell > 128 || FLAGS_redact_cell % 2 != 0) {
            cli_log() << "ERROR: --redact_cell=" << FLAGS_redact_cell << " is not an even number in [2, 128]\n";
            return false;
        }
        if (!(FLAGS_redact_margin > 0 && FLAGS_redact_margin <= 8)) {
            cli_log() << "ERROR: --redact_margin=" << FLAGS_redact_margin << " is outside (0, 8]\n";
            return false;
        }
        g_redaction.cell = FLAGS_redact_cell, g_redaction.margin = (float)FLAGS_redact_margin;
        g_redact = true;
    } else if (FLAGS_redact_only || FLAGS_redact_effect != "pixelate" || FLAGS_redact_cell != 16 || FLAGS_redact_margin != 1.0) {
        cli_log() << "ERROR: --redact_effect / --redact_cell / --redact_margin / --redact_only describe --redact=head|body\n";
        return false;
    }
    // --show_maps and its companions: enumerated names, an opacity in (0, 1], a gain above 0; the companions describe --show_maps
    if (!FLAGS_show_maps.empty()) {
        if (!pick("show_maps", FLAGS_show_maps, { { "conf", hp::map_view::max }, { "paf", hp::map_view::field } }, g_map_view.mode)
            || !pick("maps_palette", FLAGS_maps_palette, { { "jet", hp::map_view::jet }, { "heat", hp::map_view::heat }, { "grey", hp::map_view::grey } }, g_map_view.palette)
            || !pick("maps_alpha", FLAGS_maps_alpha, { { "constant", hp::map_view::constant }, { "scaled", hp::map_view::scaled } }, g_map_view.alpha))
            return false;
        if (!(FLAGS_maps_opacity > 0 && FLAGS_maps_opacity <= 1)) {
            cli_log() << "ERROR: --maps_opacity=" << FLAGS_maps_opacity << " is outside (0, 1]\n";
            return false;
        }
        if (!(FLAGS_maps_gain > 0 && FLAGS_maps_gain < 1e30)) {
            cli_log() << "ERROR: --maps_gain=" << FLAGS_maps_gain << " is not a finite number above 0\n";
            return false;
        }
        g_map_view.opacity = (float)FLAGS_maps_opacity, g_map_view.gain = (float)FLAGS_maps_gain;
        g_show_maps = true;
    } else if (FLAGS_maps_palette != "jet" || FLAGS_maps_alpha != "constant" || FLAGS_maps_opacity != 0.5 || FLAGS_maps_gain != 1.0) {
        cli_log() << "ERROR: --maps_palette / --maps_alpha / --maps_opacity / --maps_gain describe --show_maps=conf|paf\n";
        return false;
    }
    return pick("yuv_format", FLAGS_yuv_format, { { "i420", HP_YUV_I420 }, { "nv12", HP_YUV_NV12 }, { "p010", HP_YUV_P010 }, { "i010", HP_YUV_I010 },
                                                    { "nv16", HP_YUV_NV16 }, { "i422", HP_YUV_I422 }, { "yuy2", HP_YUV_YUY2 }, { "uyvy", HP_YUV_UYVY }, { "i444", HP_YUV_I444 } }, g_yuv_format)
        && pick("yuv_matrix", FLAGS_yuv_matrix, { { "bt601", HP_YUV_BT601 }, { "bt709", HP_YUV_BT709 }, { "bt2020", HP_YUV_BT2020 } }, g_yuv_matrix)
        && pick("yuv_range", FLAGS_yuv_range, { { "limited", HP_YUV_LIMITED }, { "full", HP_YUV_FULL } }, g_yuv_range);
}

// ---- media
static bool read_ppm(const std::string& path, cv::Mat& out)
{
    std::ifstream f(path, std::ios::binary);
    std::string magic;
    int w = 0, h = 0, maxv = 0;
    auto token = [&](auto& v) {
        for (;;) {
            f >> std::ws;
            if (f.peek() == '#') {
                std::string line;
                std::getline(f, line);
                continue;
            }
            f >> v;
            return;
        }
    };
    token(magic), token(w), token(h), token(maxv);
    if (!f || magic != "P6" || w <= 0 || h <= 0 || maxv != 255 || (size_t)w * h > (size_t)1 << 28)
        return false;
    f.get(); // the single whitespace after maxval
    std::vector<uint8_t> rgb((size_t)w * h * 3);
    f.read((char*)rgb.data(), rgb.size());
    if (!f)
        return false;
    out = cv::Mat(h, w, CV_8UC3);
    uint8_t* d = const_cast<uint8_t*>(hp::detail::mat_data(out));
    for (size_t i = 0; i < (size_t)w * h; ++i)
        d[i * 3] = rgb[i * 3 + 2], d[i * 3 + 1] = rgb[i * 3 + 1], d[i * 3 + 2] = rgb[i * 3]; // RGB file -> BGR cv::Mat
    return true;
}
static bool write_ppm(const std::string& path, const cv::Mat& m)
{
    std::ofstream f(path, std::ios::binary);
    f << "P6\n" << m.cols << " " << m.rows << "\n255\n";
    const uint8_t* d = hp::detail::mat_data(m);
    std::vector<uint8_t> rgb((size_t)m.rows * m.cols * 3);
    for (size_t i = 0; i < (size_t)m.rows * m.cols; ++i)
        rgb[i * 3] = d[i * 3 + 2], rgb[i * 3 + 1] = d[i * 3 + 1], rgb[i * 3 + 2] = d[i * 3];
    f.write((const char*)rgb.data(), rgb.size());
    return (bool)f;
}
static cv::Mat clone(const cv::Mat& m)
{
    cv::Mat c(m.rows, m.cols, CV_8UC3);
    std::memcpy(const_cast<uint8_t*>(hp::detail::mat_data(c)), hp::detail::mat_data(m), (size_t)m.rows * m.cols * 3);
    return c;
}
// cv::addWeighted(mat, alpha, background, 1 - alpha, 0, mat) (examples/cli.cpp:213-215): saturate_cast<uchar>(round(a * x + b * y))
static void add_weighted(cv::Mat& mat, double alpha, const cv::Mat& background)
{
    uint8_t* d = const_cast<uint8_t*>(hp::detail::mat_data(mat));
    const uint8_t* b = hp::detail::mat_data(background);
    for (size_t i = 0; i < (size_t)mat.rows * mat.cols * 3; ++i) {
        const double v = std::nearbyint(d[i] * alpha + b[i] * (1 - alpha));
        d[i] = (uint8_t)std::min(255.0, std::max(0.0, v));
    }
}
// ---- video frames (host side; the engine converts on the GPU, these helpers only make inputs and pictures to draw on)
struct yuv_buffer {
    int format = HP_YUV_NV12, matrix = HP_YUV_BT601, range = HP_YUV_LIMITED, w = 0, h = 0;
    std::vector<uint8_t> data; // hp_yuv_packed_bytes(format, w, h) bytes, tightly packed
    hp::yuv_frame frame() const { return hp::yuv_frame::packed(format, data.data(), w, h, matrix, range); }
};
static std::vector<yuv_buffer> g_yuv; // one per image, same order, when the engine is fed YUV

// ---- packed RGB / grey frames (host side, as above: inputs for the engine, BGR pictures to draw on)
struct rgb_buffer {
    int format = HP_RGB_BGR24, w = 0, h = 0;
    std::vector<uint8_t> data; // hp_rgb_packed_bytes(format, w, h) bytes, tightly packed
    hp::rgb_frame frame() const { return hp::rgb_frame::packed(format, data.data(), w, h); }
};
static std::vector<rgb_buffer> g_rgb; // one per image, same order, when the engine is fed RGB

// the BGR picture in layout `format`: memory order as the name reads, alpha 255, grey = (B + 2 G + R + 2) >> 2
static rgb_buffer bgr_to_rgb_layout(const cv::Mat& m, int format)
{
    static const char* const order[7] = { "BGR", "RGB", "BGRA", "RGBA", "ARGB", "ABGR", "Y" };
    const std::string o = order[format];
    rgb_buffer b;
    b.format = format, b.w = m.cols, b.h = m.rows;
    b.data.resize((size_t)m.cols * m.rows * o.size());
    const uint8_t* s = hp::detail::mat_data(m);
    uint8_t* d = b.data.data();
    for (size_t i = 0; i < (size_t)m.cols * m.rows; ++i, s += 3)
        for (char c : o)
            *d++ = c == 'B' ? s[0] : c == 'G' ? s[1] : c == 'R' ? s[2] : c == 'A' ? 255 : (uint8_t)((s[0] + 2 * s[1] + s[2] + 2) >> 2);
    return b;
}
static cv::Mat rgb_to_bgr(const rgb_buffer& b)
{
    cv::Mat m(b.h, b.w, CV_8UC3);
    const hp_rgb_image im = b.frame().image();
    if (hp_rgb_to_bgr_host(&im, const_cast<uint8_t*>(hp::detail::mat_data(m)), b.w * 3) != HP_OK)
        cli_log() << "ERROR: " << hp_last_error() << "\n";
    return m;
}

// BT.601 limited range, chroma = mean of its 2 x 2 pixels (what an encoder's input conversion does)
static yuv_buffer bgr_to_nv12(const cv::Mat& m)
{
    yuv_buffer out;
    out.format = HP_YUV_NV12, out.w = m.cols, out.h = m.rows;
    out.data.resize((size_t)m.cols * m.rows * 3 / 2);
    const uint8_t* d = hp::detail::mat_data(m);
    const int w = m.cols, h = m.rows;
    auto q = [](double v) { return (uint8_t)std::min(255.0, std::max(0.0, std::nearbyint(v))); };
    for (int y = 0; y < h; y += 2)
        for (int x = 0; x < w; x += 2) {
            double su = 0, sv = 0;
            for (int dy = 0; dy < 2; ++dy)
                for (int dx = 0; dx < 2; ++dx) {
                    const uint8_t* p = d + ((size_t)(y + dy) * w + x + dx) * 3;
                    const double b = p[0], g = p[1], r = p[2];
                    out.data[(size_t)(y + dy) * w + x + dx] = q(16.0 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0);
                    su += 128.0 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255.0;
                    sv += 128.0 + (112.0 * r - 93.786 * g - 18.214 * b) / 255.0;
                }
            uint8_t* c = out.data.data() + (size_t)w * h + (size_t)(y / 2) * w + x;
            c[0] = q(su / 4), c[1] = q(sv / 4);
        }
    return out;
}
// the picture the skeletons are drawn on: the frame converted on the host by the arithmetic of include/hp_hip.h with the table
// hp_yuv_coefficients returns (for I420 / NV12 at BT.601 limited range that is cv::cvtColor(COLOR_YUV2BGR_I420 / _NV12))
static cv::Mat yuv_to_bgr(const yuv_buffer& f)
{
    cv::Mat m(f.h, f.w, CV_8UC3);
    uint8_t* d = const_cast<uint8_t*>(hp::detail::mat_data(m));
    const hp::yuv_frame v = f.frame();
    if (g_hdr_on) { // an HDR frame: the picture the network is given (hp_tonemap_convert_host is the whole-frame twin of the kernels)
        const hp_yuv_image im = v.image();
        const hp_hdr_desc desc = g_hdr.c_form();
        if (hp_tonemap_convert_host(&im, &desc, d, f.w * 3) != HP_OK) {
            cli_log() << "ERROR: " << hp_last_error() << "\n";
            std::exit(-1);
        }
        return m;
    }
    const int planes = hp::yuv_frame::plane_count(f.format);
    // sample width and chroma sub-sampling as hp_yuv_plane_layout states them: bytes per luma row / width; chroma samples per row and
    // chroma rows against the luma plane's
    const bool packed = planes == 1;
    const int bytes = packed ? 1 : (int)(hp::yuv_frame::row_bytes(f.format, 0, f.w, f.h) / (size_t)f.w);
    const bool wide = bytes == 2;
    const int sx = packed || hp::yuv_frame::row_bytes(f.format, 1, f.w, f.h) / (size_t)(bytes * (planes == 2 ? 2 : 1)) != (size_t)f.w ? 1 : 0;
    const int sy = !packed && hp::yuv_frame::rows(f.format, 1, f.w, f.h) != f.h ? 1 : 0;
    int32_t k[7];
    if (hp_yuv_coefficients(f.matrix, f.range, wide ? 10 : 8, k) != HP_OK) {
        cli_log() << "ERROR: " << hp_last_error() << "\n";
        std::exit(-1);
    }
    auto sample = [&](const void* plane, size_t at) {
        const uint8_t* p = (const uint8_t*)plane + at;
        return !wide ? (int)p[0] : f.format == HP_YUV_P010 ? (p[0] | (p[1] << 8)) >> 6 : (p[0] | (p[1] << 8)) & 1023;
    };
    auto sat = [](int x) { return (uint8_t)std::min(255, std::max(0, x)); };
    for (int y = 0; y < f.h; ++y)
        for (int x = 0; x < f.w; ++x) {
            int Y, U, V;
            if (packed) { // YUY2: Y0 U Y1 V, UYVY: U Y0 V Y1
                const size_t q = (size_t)y * v.stride[0] + (size_t)(x / 2) * 4;
                const int first = f.format == HP_YUV_YUY2 ? 0 : 1;
                Y = sample(v.plane[0], q + first + (x & 1) * 2), U = sample(v.plane[0], q + 1 - first), V = sample(v.plane[0], q + 3 - first);
            } else {
                Y = sample(v.plane[0], (size_t)y * v.stride[0] + (size_t)x * bytes);
                const size_t c = (size_t)(y >> sy) * v.stride[1] + (size_t)(x >> sx) * bytes * (planes == 2 ? 2 : 1);
                U = sample(v.plane[1], c), V = planes == 2 ? sample(v.plane[1], c + bytes) : sample(v.plane[2], c);
            }
            const int yy = std::max(0, Y - k[0]) * k[2] + (1 << 19), uu = U - k[1], vv = V - k[1];
            uint8_t* p = d + ((size_t)y * f.w + x) * 3;
            p[0] = sat((yy + k[3] * uu) >> 20), p[1] = sat((yy + k[5] * vv + k[4] * uu) >> 20), p[2] = sat((yy + k[6] * vv) >> 20);
        }
    return m;
}

static std::vector<cv::Mat> load_source()
{
    std::vector<cv::Mat> images;
    auto match_suffix = [](std::string_view suffix) {
        return FLAGS_source.size() >= suffix.size() && std::equal(suffix.crbegin(), suffix.crend(), FLAGS_source.crbegin());
    };
    if (FLAGS_source.rfind("synthetic:", 0) == 0) {
        int n = 0, w = 0, h = 0;
        if (std::sscanf(FLAGS_source.c_str(), "synthetic:%d:%dx%d", &n, &w, &h) != 3 || n <= 0 || w <= 0 || h <= 0 || n > 4096)
            return {};
        unsigned s = 20240;
        for (int i = 0; i < n; ++i) {
            cv::Mat m(h, w, CV_8UC3);
            uint8_t* d = const_cast<uint8_t*>(hp::detail::mat_data(m));
            for (size_t k = 0; k < (size_t)w * h * 3; ++k)
                s = s * 1664525u + 1013904223u, d[k] = (uint8_t)(s >> 24);
            images.push_back(m);
        }
        return images;
    }
#ifdef HYPERPOSE_USE_OPENCV
    if (match_suffix(".jpg") || match_suffix(".jpeg") || match_suffix(".png"))
        return { cv::imread(FLAGS_source) };
#endif
    if (match_suffix(".yuv")) { // raw frames of --yuv_format, back to back
        const size_t bytes = hp_yuv_packed_bytes(g_yuv_format, FLAGS_yuv_w, FLAGS_yuv_h);
        if (bytes == 0) {
            cli_log() << "ERROR: a .yuv source needs --yuv_w and --yuv_h (even numbers for 4:2:0, an even width for 4:2:2): raw video carries no header\n";
            return {};
        }
        std::ifstream f(FLAGS_source, std::ios::binary | std::ios::ate);
        const std::streamoff size = f ? (std::streamoff)f.tellg() : 0;
        if (size <= 0 || (size_t)size % bytes != 0) {
            cli_log() << "ERROR: " << FLAGS_source << " holds " << size << " bytes, which is not a whole number of " << FLAGS_yuv_format << " frames of "
                      << FLAGS_yuv_w << " x " << FLAGS_yuv_h << " (" << bytes << " bytes each)\n";
            return {};
        }
        f.seekg(0);
        for (;;) {
            yuv_buffer b;
            b.format = g_yuv_format, b.matrix = g_yuv_matrix, b.range = g_yuv_range, b.w = FLAGS_yuv_w, b.h = FLAGS_yuv_h;
            b.data.resize(bytes);
            if (!f.read((char*)b.data.data(), bytes))
                break;
            images.push_back(yuv_to_bgr(b));
            g_yuv.push_back(std::move(b));
        }
        FLAGS_yuv = g_yuv_from_file = true;
        return images;
    }
    if (match_suffix(".rgb")) { // raw frames of --rgb=<layout>, --yuv_w x --yuv_h, back to back
        const size_t bytes = hp_rgb_packed_bytes(g_rgb_format, FLAGS_yuv_w, FLAGS_yuv_h);
        if (bytes == 0) {
            cli_log() << "ERROR: a .rgb source needs --yuv_w and --yuv_h: raw frames carry no header\n";
            return {};
        }
        std::ifstream f(FLAGS_source, std::ios::binary | std::ios::ate);
        const std::streamoff size = f ? (std::streamoff)f.tellg() : 0;
        if (size <= 0 || (size_t)size % bytes != 0) {
            cli_log() << "ERROR: " << FLAGS_source << " holds " << size << " bytes, which is not a whole number of " << FLAGS_rgb << " frames of " << FLAGS_yuv_w
                      << " x " << FLAGS_yuv_h << " (" << bytes << " bytes each)\n";
            return {};
        }
        f.seekg(0);
        for (;;) {
            rgb_buffer b;
            b.format = g_rgb_format, b.w = FLAGS_yuv_w, b.h = FLAGS_yuv_h;
            b.data.resize(bytes);
            if (!f.read((char*)b.data.data(), bytes))
                break;
            images.push_back(rgb_to_bgr(b));
            g_rgb.push_back(std::move(b));
        }
        return images;
    }
    if (match_suffix(".ppm")) {
        cv::Mat m;
        if (read_ppm(FLAGS_source, m))
            images.push_back(m);
        return images;
    }
    if (DIR* dir = opendir(FLAGS_source.c_str())) { // glob_images (examples/utils.cpp)
        std::vector<std::string> names;
        while (dirent* e = readdir(dir))
            names.push_back(e->d_name);
        closedir(dir);
        std::sort(names.begin(), names.end());
        for (const auto& nm : names) {
            cv::Mat m;
            const std::string path = FLAGS_source + "/" + nm;
            if (nm.size() > 4 && nm.substr(nm.size() - 4) == ".ppm" && read_ppm(path, m))
                images.push_back(m);
#ifdef HYPERPOSE_USE_OPENCV
            else if (!(m = cv::imread(path)).empty())
                images.push_back(m);
#endif
        }
    }
    return images;
}

// --synthetic_humans: n humans of frame `frame`, every part but a few present, spread over the picture (and a little beyond it)
static void add_synthetic_humans(std::vector<hp::human_t>& poses, size_t frame, int n)
{
    unsigned s = 9001u + (unsigned)frame * 7919u;
    auto next = [&] { return (s = s * 1664525u + 1013904223u, (float)(s >> 8) / (float)(1 << 24)); };
    for (int i = 0; i < n; ++i) {
        hp::human_t h{};
        h.score = 1;
        const float cx = 0.05f + 0.9f * next(), cy = 0.1f + 0.8f * next();
        for (int k = 0; k < hp::COCO_N_PARTS; ++k) {
            const float x = cx + 0.2f * (next() - 0.5f), y = cy + 0.4f * (next() - 0.5f);
            if (next() < 0.85f)
                h.parts[k] = hp::body_part_t{ true, x, y, 1.f };
        }
        poses.push_back(h);
    }
}

// the three post-processing operators behind one value (the `--post` flag picks the alternative)
using any_parser = std::variant<hp::parser::paf, hp::parser::pose_proposal, hp::parser::pifpaf>;

static bool has_suffix(const std::string& text, std::string_view suffix)
{
    return text.size() >= suffix.size() && text.compare(text.size() - suffix.size(), suffix.size(), suffix) == 0;
}

// `--model`: built-in topology with synthetic weights, ONNX file, UFF file (TensorFlow frozen graphs: refused by the engine with its
// own message), or - any other name - an engine saved with tensorrt::save
static hp::dnn::tensorrt build_engine()
{
    const cv::Size net_size(FLAGS_w, FLAGS_h);
    cli_log() << "engine: model '" << FLAGS_model << "', network input " << FLAGS_w << " x " << FLAGS_h << " (w x h), batches of up to "
              << FLAGS_max_batch_size << (FLAGS_keep_ratio ? ", aspect ratio kept (letter-box)\n" : ", frames stretched to the network size\n");
    const hp::data_type dtype = FLAGS_int8 ? hp::data_type::kINT8 : FLAGS_half ? hp::data_type::kHALF : hp::data_type::kFLOAT;
    if (FLAGS_model.rfind("builtin:", 0) == 0)
        return hp::dnn::tensorrt(hp::dnn::builtin_model{ FLAGS_model.substr(8), {}, 20241 }, net_size, FLAGS_max_batch_size, FLAGS_keep_ratio, dtype);
    if (has_suffix(FLAGS_model, ".onnx"))
        return hp::dnn::tensorrt(hp::dnn::onnx{ FLAGS_model }, net_size, FLAGS_max_batch_size, FLAGS_keep_ratio, dtype);
    if (has_suffix(FLAGS_model, ".uff"))
        return hp::dnn::tensorrt(hp::dnn::uff{ FLAGS_model, "image", { "outputs/conf", "outputs/paf" } }, net_size, FLAGS_max_batch_size, FLAGS_keep_ratio);
    cli_log() << "'" << FLAGS_model << "' is neither .onnx nor .uff: loading it as a serialized engine\n";
    return hp::dnn::tensorrt(hp::dnn::tensorrt_serialized{ FLAGS_model }, net_size, FLAGS_max_batch_size, FLAGS_keep_ratio);
}

static any_parser build_parser(hp::dnn::tensorrt& engine) // (input_size() is non-const in the reference's class, tensorrt.hpp:98)
{
    const cv::Size in = engine.input_size();
    if (FLAGS_post == kPPN)
        return any_parser{ std::in_place_type<hp::parser::pose_proposal>, in };
    if (FLAGS_post == kPIFPAF)
        return any_parser{ std::in_place_type<hp::parser::pifpaf>, in.height, in.width };
    if (FLAGS_post != kPAF) {
        cli_log() << "ERROR: --post=" << FLAGS_post << " is not one of " kPAF ", " kPPN ", " kPIFPAF "\n";
        std::exit(-1);
    }
    return any_parser{ std::in_place_type<hp::parser::paf> };
}

int main(int argc, char** argv)
{
    if (!parse_flags(argc, argv))
        return 1;
    if (FLAGS_logging)
        cli_log() << "--logging: the engine reports through hp_last_error(); nothing more to switch on\n";
    if (FLAGS_alpha < 0 || FLAGS_alpha > 1) {
        const double inside = std::min(1.0, std::max(0.0, FLAGS_alpha));
        cli_log() << "WARNING: --alpha=" << FLAGS_alpha << " is outside [0, 1]; using " << inside << "\n";
        FLAGS_alpha = inside;
    }
    // --saving_yuv is settled from the flags alone, before anything touches the device
    if (!FLAGS_saving_yuv.empty() && !FLAGS_yuv && !has_suffix(FLAGS_source, ".yuv")) {
        cli_log() << "ERROR: --saving_yuv writes video frames: it needs a .yuv source or --yuv\n";
        return 1;
    }
    // --redact rewrites the frames --saving_yuv writes: settled from the flags alone as well
    if (g_redact && FLAGS_saving_yuv.empty() && FLAGS_encode_yuv.empty()) {
        cli_log() << "ERROR: --redact=" << FLAGS_redact << " redacts the frames of --saving_yuv=<file>; the PPM pictures are not redacted\n";
        return 1;
    }
    // --show_maps blends the network's maps into the frames --saving_yuv writes, in the operator runtime (the stream runtime recycles its engine
    // outputs before the caller holds the humans), from the conf / paf pair of a PAF network, one engine call per frame batch (no tiles)
    if (g_show_maps && FLAGS_saving_yuv.empty()) {
        cli_log() << "ERROR: --show_maps=" << FLAGS_show_maps << " shows the maps on the frames of --saving_yuv=<file>; the PPM pictures do not get them\n";
        return 1;
    }
    if (g_show_maps && FLAGS_runtime == kSTREAM) {
        cli_log() << "ERROR: --show_maps=" << FLAGS_show_maps << " needs --runtime=" kOPERATOR ": with --runtime=" kSTREAM " the engine's outputs are recycled before the humans arrive\n";
        return 1;
    }
    if (g_show_maps && (FLAGS_post != kPAF || !FLAGS_tiles.empty())) {
        cli_log() << "ERROR: --show_maps=" << FLAGS_show_maps << " shows the conf / paf maps of one engine call per frame: --post=" kPAF " without --tiles\n";
        return 1;
    }
    // --flip_ensemble is settled from the flags alone too: the PAF maps are the ones with a left / right channel table
    if (FLAGS_flip_ensemble && FLAGS_post != kPAF) {
        cli_log() << "ERROR: --flip_ensemble merges the maps of a PAF network (--post=" kPAF "), got --post=" << FLAGS_post << "\n";
        return 1;
    }
    if (FLAGS_flip_ensemble && (g_tiled ? 2 * g_tiling.regions() : 2) > FLAGS_max_batch_size) {
        cli_log() << "ERROR: --flip_ensemble runs every " << (g_tiled ? "region" : "frame") << " with its flip: " << (g_tiled ? 2 * g_tiling.regions() : 2)
                  << " network images per frame, more than --max_batch_size=" << FLAGS_max_batch_size << "\n";
        return 1;
    }
    // --scale_ensemble likewise: 1 .. 3 scales in (0, 1], a PAF network, and room for every pass of a frame
    if (!FLAGS_scale_ensemble.empty()) {
        const std::string list = FLAGS_scale_ensemble + ",";
        bool ok = true;
        for (size_t at = 0, comma; ok && (comma = list.find(',', at)) != std::string::npos; at = comma + 1) {
            const std::string item = list.substr(at, comma - at);
            char* end = nullptr;
            const float v = std::strtof(item.c_str(), &end);
            ok = !item.empty() && *end == 0 && v > 0.f && v <= 1.f && g_scales.size() < 3; // (nan fails both comparisons)
            g_scales.push_back(v);
        }
        if (!ok) {
            cli_log() << "ERROR: --scale_ensemble=" << FLAGS_scale_ensemble << ": expected 1 .. 3 comma-separated scales in (0, 1], e.g. 0.5,0.75\n";
            return 1;
        }
        if (FLAGS_post != kPAF) {
            cli_log() << "ERROR: --scale_ensemble merges the maps of a PAF network (--post=" kPAF "), got --post=" << FLAGS_post << "\n";
            return 1;
        }
        const int passes = (int)(g_scales.size() + 1) * (FLAGS_flip_ensemble ? 2 : 1) * (g_tiled ? g_tiling.regions() : 1);
        if (passes > FLAGS_max_batch_size) {
            cli_log() << "ERROR: --scale_ensemble runs every " << (g_tiled ? "region" : "frame") << " at " << g_scales.size() + 1 << " scales"
                      << (FLAGS_flip_ensemble ? " with their flips" : "") << ": " << passes << " network images per frame, more than --max_batch_size="
                      << FLAGS_max_batch_size << "\n";
            return 1;
        }
    }
    if (g_tiled && g_tiling.regions() > FLAGS_max_batch_size) {
        cli_log() << "ERROR: --tiles=" << FLAGS_tiles << (FLAGS_tile_full ? " --tile_full" : "") << " makes " << g_tiling.regions()
                  << " regions per frame, more than --max_batch_size=" << FLAGS_max_batch_size << "\n";
        return 1;
    }
    if (FLAGS_synthetic_humans > 0)
        cli_log() << "WARNING: --synthetic_humans=" << FLAGS_synthetic_humans << ": " << FLAGS_synthetic_humans
                  << " made-up humans are added to every frame's poses; the pictures and the human count below are NOT the model's result\n";
    if (hp_init(0) != HP_OK) {
        cli_log() << "ERROR: " << hp_last_error() << "\n";
        return 2;
    }
    auto images = load_source();
    if (images.empty()) {
        cli_log() << "ERROR: no frames from --source=" << FLAGS_source << " (PPM files / directories and synthetic:<n>:<w>x<h> are supported"
#ifndef HYPERPOSE_USE_OPENCV
                  << "; videos and the camera need a build with OpenCV"
#endif
                  << ")" << std::endl;
        std::exit(-1);
    }
    if (FLAGS_yuv && g_yuv.empty()) { // --yuv on a BGR source: the frames as a hardware decoder would deliver them
        for (const auto& m : images) {
            if (m.cols % 2 || m.rows % 2) {
                cli_log() << "ERROR: --yuv needs frames of even width and height (4:2:0), got " << m.cols << " x " << m.rows << "\n";
                return 1;
            }
            g_yuv.push_back(bgr_to_nv12(m));
        }
    }
    if (g_rgb_format >= 0 && g_rgb.empty()) // --rgb on a BGR source: the frames as a capture API or a grey camera would deliver them
        for (const auto& m : images)
            g_rgb.push_back(bgr_to_rgb_layout(m, g_rgb_format));
    if (g_rgb_format >= 0 && FLAGS_runtime == kSTREAM) {
        cli_log() << "WARNING: the stream runtime carries cv::Mat frames (stream.hpp); RGB frames go through --runtime=" kOPERATOR "\n";
        FLAGS_runtime = kOPERATOR;
    }
    if (FLAGS_yuv && FLAGS_runtime == kSTREAM) {
        cli_log() << "WARNING: the stream runtime carries cv::Mat frames (stream.hpp); YUV frames go through --runtime=" kOPERATOR "\n";
        FLAGS_runtime = kOPERATOR;
    }
    if (!FLAGS_encode_yuv.empty() && FLAGS_runtime == kSTREAM) {
        cli_log() << "WARNING: the stream runtime returns humans, not frames; --encode_yuv goes through --runtime=" kOPERATOR "\n";
        FLAGS_runtime = kOPERATOR;
    }
    std::ofstream yuv_out, humans_out, encode_out, encode_humans_out;
    if (!FLAGS_encode_yuv.empty()) {
        encode_out.open(FLAGS_encode_yuv, std::ios::binary | std::ios::trunc);
        encode_humans_out.open(FLAGS_encode_yuv + ".humans", std::ios::binary | std::ios::trunc);
        if (!encode_out || !encode_humans_out) {
            cli_log() << "ERROR: cannot write " << FLAGS_encode_yuv << "\n";
            return 1;
        }
    }
    if (!FLAGS_saving_yuv.empty()) {
        yuv_out.open(FLAGS_saving_yuv, std::ios::binary | std::ios::trunc);
        humans_out.open(FLAGS_saving_yuv + ".humans", std::ios::binary | std::ios::trunc);
        if (!yuv_out || !humans_out) {
            cli_log() << "ERROR: cannot write " << FLAGS_saving_yuv << "\n";
            return 1;
        }
    }
    if (FLAGS_imshow) {
        FLAGS_imshow = false;
        cli_log() << "--imshow needs a display and OpenCV's highgui: results go to files only\n";
    }

    auto engine = build_engine();
    if (g_hdr_on)
        engine.set_tonemap(g_hdr);
    engine.set_orientation(g_orient); // (from here on every frame the engine is given is a stored frame, calibration frames included)
    if (FLAGS_int8 && !engine.calibrated()) { // calibration is never implicit in the engine: the CLI asks for it and says so
        const size_t n = std::min(images.size(), (size_t)FLAGS_max_batch_size);
        if (FLAGS_yuv) {
            std::vector<hp::yuv_frame> frames;
            for (size_t i = 0; i < n; ++i)
                frames.push_back(g_yuv[i].frame());
            engine.calibrate(frames);
        } else if (g_rgb_format >= 0) {
            std::vector<hp::rgb_frame> frames;
            for (size_t i = 0; i < n; ++i)
                frames.push_back(g_rgb[i].frame());
            engine.calibrate(frames);
        } else
            engine.calibrate(std::vector<cv::Mat>(images.begin(), images.begin() + n));
        std::cerr << "--int8: calibrated the kINT8 engine on the first " << n << " frame(s) of the source (MinMax)" << std::endl;
    }
    any_parser parser = build_parser(engine);
    if (FLAGS_flip_ensemble && FLAGS_runtime != kSTREAM) { // (after the calibration, which runs the plain schedule; the stream sets its own engines)
        engine.set_flip_ensemble(true);
        cli_log() << "--flip_ensemble: every frame runs with its left-right flip, batches of up to " << engine.batch_room() << "\n";
    }
    if (!g_scales.empty() && FLAGS_runtime != kSTREAM) { // (after the calibration, as the flip ensemble)
        engine.set_scale_ensemble(g_scales);
        cli_log() << "--scale_ensemble: every frame runs at " << g_scales.size() + 1 << " scales, batches of up to " << engine.batch_room() << "\n";
    }
    if (FLAGS_runtime != kOPERATOR && FLAGS_runtime != kSTREAM) {
        cli_log() << "WARNING: --runtime=" << FLAGS_runtime << " is neither " kOPERATOR " nor " kSTREAM "; using " kOPERATOR "\n";
        FLAGS_runtime = kOPERATOR;
    }

    using clk_t = std::chrono::high_resolution_clock;
    size_t n_humans = 0, n_written = 0;
    // `img` is the picture as stored, `poses` are normalised to the upright frame: resume_ratio runs on the upright size, to_stored brings
    // the records to the picture
    auto render = [&](cv::Mat& img, std::vector<hp::human_t> poses, bool resume) {
        cv::Mat background;
        if (FLAGS_alpha > 0)
            background = clone(img);
        if (resume)
            for (auto& pose : poses)
                hp::resume_ratio(pose, hp::oriented_size(img.size(), g_orient), engine.input_size());
        hp::to_stored(poses, g_orient);
        for (const auto& pose : poses)
            hp::draw_human(img, pose);
        if (FLAGS_alpha > 0)
            add_weighted(img, FLAGS_alpha, background);
        n_humans += poses.size();
        n_written += write_ppm(FLAGS_saving_prefix + "_" + std::to_string(n_written) + ".ppm", img);
    };

    // --tiles: one frame's regions in one engine call, every region parsed on its own, the poses brought back to the frame and merged
    // (with --rotate / --hflip the regions, and the poses returned, are in the upright frame's coordinates)
    auto tiled_poses = [&](const cv::Mat& stored, const hp::yuv_frame* yuv, const hp::rgb_frame* rgb = nullptr) {
        const cv::Size frame = hp::oriented_size(stored.size(), g_orient);
        const std::vector<cv::Rect> regions = hp::plan_tiles(frame, g_tiling, yuv ? yuv->format : -1, g_orient);
        const auto maps = yuv ? engine.inference(*yuv, regions) : rgb ? engine.inference(*rgb, regions) : engine.inference(stored, regions);
        std::vector<hp::human_t> all;
        std::vector<int> region_of;
        for (size_t r = 0; r < regions.size(); ++r)
            for (auto pose : std::visit([&](auto& op) { return op.process(maps[r]); }, parser)) {
                if (FLAGS_keep_ratio)
                    hp::resume_ratio(pose, cv::Size(regions[r].width, regions[r].height), engine.input_size());
                hp::to_frame(pose, regions[r], frame);
                all.push_back(pose), region_of.push_back((int)r);
            }
        return regions.size() == 1 ? all : hp::merge_humans(all, region_of, frame, g_tiling.min_common, g_tiling.tol);
    };

    auto beg = clk_t::now();
    if (FLAGS_runtime == kOPERATOR) {
        // operator API: one batch at a time - engine.inference(batch) -> one internal_t per frame -> parser.process(internal_t)
        const size_t step = std::max<size_t>(1, engine.batch_room());
        for (size_t first = 0; first < images.size(); first += step) {
            std::vector<cv::Mat> batch(images.begin() + first, images.begin() + std::min(images.size(), first + step));
            std::vector<hp::yuv_frame> yuv_batch;
            std::vector<std::unique_ptr<hp::detail::dev_ptr>> surfaces; // --saving_yuv: the frames as device-resident surfaces
            if (FLAGS_yuv)
                for (size_t k = 0; k < batch.size(); ++k) {
                    const yuv_buffer& b = g_yuv[first + k];
                    if (!yuv_out.is_open()) {
                        yuv_batch.push_back(b.frame());
                        continue;
                    }
                    surfaces.push_back(std::make_unique<hp::detail::dev_ptr>(b.data.size()));
                    if (!surfaces.back()->p || hp_memcpy_h2d(surfaces.back()->p, b.data.data(), b.data.size()) != HP_OK) {
                        cli_log() << "ERROR: " << hp_last_error() << "\n";
                        return 2;
                    }
                    yuv_batch.push_back(hp::yuv_frame::packed(b.format, surfaces.back()->p, b.w, b.h, b.matrix, b.range, true));
                }
            std::vector<hp::rgb_frame> rgb_batch;
            if (g_rgb_format >= 0)
                for (size_t k = 0; k < batch.size(); ++k)
                    rgb_batch.push_back(g_rgb[first + k].frame());
            const auto maps = g_tiled ? std::vector<hp::internal_t>{}
                : FLAGS_yuv       ? engine.inference(yuv_batch)
                : g_rgb_format >= 0 ? engine.inference(rgb_batch)
                                    : engine.inference(batch);
            for (size_t k = 0; k < batch.size(); ++k) {
                auto poses = g_tiled ? tiled_poses(batch[k], FLAGS_yuv ? &yuv_batch[k] : nullptr, g_rgb_format >= 0 ? &rgb_batch[k] : nullptr) : std::visit([&](auto& op) { return op.process(maps[k]); }, parser);
                add_synthetic_humans(poses, first + k, FLAGS_synthetic_humans);
                if (yuv_out.is_open()) { // annotate the surface where it lies, in its own format, and append it to the file
                    std::vector<hp::human_t> drawn = poses;
                    if (FLAGS_keep_ratio && !g_tiled) // (tiled poses are in the frame's coordinates already)
                        for (auto& pose : drawn)
                            hp::resume_ratio(pose, hp::oriented_size(batch[k].size(), g_orient), engine.input_size());
                    // `drawn` stays upright (it is what <file>.humans records); the surface is the stored frame
                    if (g_redact) // first the persons made unrecognisable, then the skeletons on top
                        hp::redact_humans(yuv_batch[k], drawn, g_orient, g_redaction);
                    if (g_show_maps) // then what the network saw, under the skeletons: maps[k] = (conf, paf) of this frame, still on the device
                        hp::draw_maps(yuv_batch[k], maps[k][g_map_view.mode == hp::map_view::field ? 1 : 0],
                            engine.map_cover(hp::oriented_size(batch[k].size(), g_orient)), g_orient, g_map_view);
                    if (!FLAGS_redact_only) {
                        if (g_hdr_on)
                            hp::draw_humans(yuv_batch[k], drawn, g_orient, g_hdr, FLAGS_alpha > 0 ? (float)FLAGS_alpha : 1.f);
                        else
                            hp::draw_humans(yuv_batch[k], drawn, g_orient, FLAGS_alpha > 0 ? (float)FLAGS_alpha : 1.f);
                    }
                    std::vector<uint8_t> annotated(g_yuv[first + k].data.size());
                    if (hp_device_synchronize() != HP_OK || hp_memcpy_d2h(annotated.data(), surfaces[k]->p, annotated.size()) != HP_OK) {
                        cli_log() << "ERROR: " << hp_last_error() << "\n";
                        return 2;
                    }
                    yuv_out.write((const char*)annotated.data(), annotated.size());
                    const auto records = hp::detail::to_c_humans(drawn);
                    const int32_t count = (int32_t)records.size();
                    humans_out.write((const char*)&count, sizeof(count));
                    humans_out.write((const char*)records.data(), records.size() * sizeof(hp_human));
                }
                if (encode_out.is_open()) { // the frame in its own layout -> device -> the encoder's frame, annotated where it lies, appended to the file
                    const cv::Mat& m = batch[k];
                    const hp::rgb_frame host = g_rgb_format >= 0 ? rgb_batch[k] : hp::rgb_frame(HP_RGB_BGR24, hp::detail::mat_data(m), m.cols, m.rows, m.cols * 3);
                    const cv::Size size = hp::padded_size(g_encode_format, cv::Size(host.width, host.height), FLAGS_encode_align);
                    std::vector<uint8_t> encoded(hp_yuv_packed_bytes(g_encode_format, size.width, size.height));
                    hp::detail::dev_ptr src((size_t)host.stride * host.height), dst(encoded.size());
                    if (!src.p || !dst.p || hp_memcpy_h2d(src.p, host.data, (size_t)host.stride * host.height) != HP_OK) {
                        cli_log() << "ERROR: " << hp_last_error() << "\n";
                        return 2;
                    }
                    hp::yuv_frame surface = hp::yuv_frame::packed(g_encode_format, dst.p, size.width, size.height, g_encode_matrix, g_encode_range, true);
                    hp::to_yuv(hp::rgb_frame(host.format, src.p, host.width, host.height, host.stride, true), surface);
                    std::vector<hp::human_t> drawn = poses; // upright, normalised to the source frame: what <file>.humans records
                    if (FLAGS_keep_ratio && !g_tiled)
                        for (auto& pose : drawn)
                            hp::resume_ratio(pose, hp::oriented_size(m.size(), g_orient), engine.input_size());
                    // the surface is the stored frame with padding on its right and below: stored coordinates, rescaled to the padded size
                    std::vector<hp::human_t> on_surface = drawn;
                    hp::to_stored(on_surface, g_orient);
                    const float fx = (float)host.width / (float)size.width, fy = (float)host.height / (float)size.height;
                    for (auto& pose : on_surface)
                        for (auto& part : pose.parts)
                            part.x *= fx, part.y *= fy;
                    if (g_redact)
                        hp::redact_humans(surface, on_surface, g_redaction);
                    if (!FLAGS_redact_only)
                        hp::draw_humans(surface, on_surface, FLAGS_alpha > 0 ? (float)FLAGS_alpha : 1.f);
                    if (hp_device_synchronize() != HP_OK || hp_memcpy_d2h(encoded.data(), dst.p, encoded.size()) != HP_OK) {
                        cli_log() << "ERROR: " << hp_last_error() << "\n";
                        return 2;
                    }
                    encode_out.write((const char*)encoded.data(), encoded.size());
                    const auto records = hp::detail::to_c_humans(drawn);
                    const int32_t count = (int32_t)records.size();
                    encode_humans_out.write((const char*)&count, sizeof(count));
                    encode_humans_out.write((const char*)records.data(), records.size() * sizeof(hp_human));
                }
                render(batch[k], poses, FLAGS_keep_ratio && !g_tiled);
            }
        }
    } else {
        // stream API: make_stream(engine, parser, use_original_resolution = true, keep_ratio); frames in, (frame, poses) out in order
        std::visit(
            [&](auto& op) {
                auto stream = hp::make_stream(engine, op, true, FLAGS_keep_ratio);
                if (g_tiled)
                    stream.set_tiling(g_tiling);
                stream.set_orientation(g_orient);
                if (FLAGS_flip_ensemble)
                    stream.set_flip_ensemble(true);
                if (!g_scales.empty())
                    stream.set_scale_ensemble(g_scales);
                stream.async() << images;
                auto sink = [&](size_t, const cv::Mat& frame, const std::vector<hp::human_t>& poses) {
                    cv::Mat img = clone(frame);
                    render(img, poses, false); // the stream already applied resume_ratio
                };
                stream.sync() >> sink;
            },
            parser);
    }
    const auto ms = std::chrono::duration<double, std::milli>(clk_t::now() - beg).count();
    std::cout << images.size() << " images got processed in " << ms << " ms, FPS = " << 1000. * images.size() / ms << " (" << n_humans
              << " humans, " << n_written << " files written as " << FLAGS_saving_prefix << "_<id>.ppm)\n";
    if (yuv_out.is_open()) {
        yuv_out.flush(), humans_out.flush();
        if (!yuv_out || !humans_out) {
            cli_log() << "ERROR: writing " << FLAGS_saving_yuv << " failed\n";
            return 3;
        }
        std::cout << images.size() << " annotated " << FLAGS_yuv_format_written() << " frames appended to " << FLAGS_saving_yuv << "\n";
    }
    if (encode_out.is_open()) {
        encode_out.flush(), encode_humans_out.flush();
        if (!encode_out || !encode_humans_out) {
            cli_log() << "ERROR: writing " << FLAGS_encode_yuv << " failed\n";
            return 3;
        }
        std::cout << images.size() << " " << FLAGS_encode_format << " frames (" << FLAGS_encode_matrix << ", " << FLAGS_encode_range << ") appended to " << FLAGS_encode_yuv << "\n";
    }
    return n_written == images.size() ? 0 : 3;
}
