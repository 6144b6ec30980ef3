"""``native/tools/gemm_bench_report.h``: mx-gemm-bench's RESULT lines, pass rule
and spot block against recorded strings (no GPU)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_test_of_the_report_header():
    """make test-gemm-bench-report: the five recorded result lines, both
    allocation-failure lines, the pass rule's table and the spot blocks, under
    ASan + UBSan."""
    p = subprocess.run(["make", "-C", REPO, "test-gemm-bench-report"], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "every line equal to the recorded one" in p.stdout
