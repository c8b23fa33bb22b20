"""The negotiation's protocol unit on its own (tips_amd/csrc/neg_protocol.{h,cc}): record codecs,
rank 0's table and decision, the response cache and the linger's expected set, driven by
tests/c/neg_protocol_check.cc with p simulated ranks in one process - chosen announce sequences in
front of the decision, which the multi-process tests (test_negotiation_cpu.py) cannot place.

tools/_bin/neg_protocol_check is that program built from neg_protocol.cc and err.cc alone (it
linking without HIP or RCCL shows the unit has neither) under AddressSanitizer and UBSan, so the
malformed-input cases also show that a rejected message was rejected without reading out of bounds."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "tools", "_bin", "neg_protocol_check")


def test_protocol_unit_checks_pass_under_sanitizers():
    assert os.path.exists(BIN), "tools/_bin/neg_protocol_check missing: run make"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    assert "checks ok" in r.stdout, out
    for word in ("Sanitizer", "runtime error", "CHECK failed"):
        assert word not in out, out
