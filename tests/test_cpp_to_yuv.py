"""CPU: the encoder hand-off from C++.  (1) hyperpose::to_yuv / hyperpose::padded_size (include/hyperpose/utility/encode.hpp) compile with plain g++
against the mirror headers and give, on a host rgb_frame and on a cv::Mat, the bytes of hp_rgb_to_yuv_host (tests/cpp/to_yuv_api.cpp).  (2) The host
side of hyperpose_amd/csrc/to_yuv.hpp as a stand-alone program built with g++ -fsanitize=address,undefined on sources and planes allocated with no
slack (tests/cpp/to_yuv_rules.cpp): a read outside a row's pixels, a write outside a plane's samples or an overflow in the integer rules aborts it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_to_yuv_mirror_on_host_frames():
    src, exe = os.path.join(CPP, "to_yuv_api.cpp"), os.path.join(CPP, "to_yuv_api.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-L" + os.path.join(ROOT, "hyperpose_amd"),
                           "-lhp_hip", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    # 5 layouts x (an ARGB frame with a pitch, a cv::Mat); four refusals
    assert out.stdout.split()[-3:] == ["OK", "10", "4"]


def test_to_yuv_rules_stay_inside_their_buffers_under_sanitizers():
    src, exe = os.path.join(CPP, "to_yuv_rules.cpp"), os.path.join(CPP, "to_yuv_rules.bin")
    # the sanitizers' runtimes are linked statically: the program needs nothing of its environment to start
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-4000:]
    # the table and 4 padded sizes; 9 x 7 layout pairs x 5 sizes x 5 checks; 12 tables of grey; 4 size rules
    assert out.stdout.split() == ["OK", str(1 + 4 + 9 * 7 * 5 * 5 + 12 + 4)]
