"""The workspace plan (n-hans_amd/csrc/ws_plan.h) on the host: tests/ws_plan_main.cpp includes the header alone, places plans
over a host array and checks every slot, the total, zero counts, mark / rewind, a plan that is never placed and the fixed
capacity.  Built with the address and undefined-behaviour sanitizers and run as a plain child process: exit status 0."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_ws_plan_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ws_plan_main")
    # (the sanitizer runtimes are linked statically, so the program needs no preload)
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", os.path.join(HERE, "ws_plan_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
