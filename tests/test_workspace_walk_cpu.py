"""csrc/workspace.h, the one walk that sizes and carves every device workspace, checked on the host: tests/workspace_walk.cpp includes the
header alone (it is plain C++ without HIP types) and runs a measuring walk against a real one over a few region lists."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "large-steps-pytorch_amd", "csrc")


def test_measuring_and_real_walk_agree(tmp_path):
    exe = tmp_path / "workspace_walk"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "workspace_walk.cpp"), "-o", str(exe)],
                   check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stderr


def test_the_rounding_lives_in_the_header_alone():
    """no other file of csrc/ rounds a size or an offset up to 256 by hand (the base pointer's rounding is ws_align_base)"""
    found = []
    for name in sorted(os.listdir(CSRC)):
        if name == "workspace.h" or not name.endswith((".h", ".hip", ".cpp")):
            continue
        for no, line in enumerate(open(os.path.join(CSRC, name)), 1):
            text = line.replace(" ", "")
            if "&~(size_t)255" in text or "&~size_t(255)" in text or "&~(uintptr_t)255" in text or "autoal=" in text:
                found.append(f"{name}:{no}")
    assert not found, found
