"""The cooperative mode's policy (tc-viml_amd/csrc/tcv_coop_policy.cpp) without a device: the helper count of a batch and the per-XCD
admission table of cooperative launches, pinned by tests/dev/coop_policy_check.cpp at the points where they decide -- five one-group
launches rotating over the XCDs, the fifth eight-group launch refused with the table untouched, the ninth group wrapping onto the first
one's XCD, one CU per XCD, two devices; the helper count at its factor, window and CU thresholds.  Plain g++, no HIP include path, under
AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_coop_policy_compiles_without_hip_and_holds_its_pins_under_sanitizers(tmp_path):
    exe = str(tmp_path / "coop_policy_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "dev", "coop_policy_check.cpp"),
                           os.path.join(ROOT, "tc-viml_amd", "csrc", "tcv_coop_policy.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "coop_policy_check: ok" and out.stderr == ""
