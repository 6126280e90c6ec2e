"""The res2 stage launch (C = 64), host side, no GPU: the weight stream pack_stage1_c64_stream (api_chain.hip) builds, walked with the wave
layout conv_stage1_c64_kernel reads it with (tests/cpp/stage_c64_pack_check.cpp) - every weight byte of the block's three convolutions
appears exactly once, at the fragment, lane and byte the kernel's MFMA operands take it from.

That the optimiser forms the site for ResNet50 and leaves it off needs a device: the stream is uploaded, and the site formed, only where the
placement probe (workgroup b on XCD b % 8) holds, which no host-only runtime answers. tests/test_gpu_stage_c64.py::
test_resnet50_net_runs_res2_as_one_launch asserts it."""
import os
import subprocess

from anakin_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))


def test_packed_stream_against_the_oihw_weights():
    exe = os.path.join(HERE, "cpp", "stage_c64_pack_check.bin")
    if not os.path.exists(exe) or os.path.exists("/opt/rocm/bin/hipcc"):
        B.build_cpp_tests()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "stage c64 stream ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])

