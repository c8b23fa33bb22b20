"""tools/stream_order_diff.py on small hand-written traces: other pointers' worth of stream ids,
thread ids, correlation ids and timestamps compare equal; a wait that moved past a launch, a
launch on another stream and a changed grid are each reported."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tools", "stream_order_diff.py")
CALLS = ["hipEventRecord", "hipStreamWaitEvent", "hipLaunchKernel:pack:96:7", "hipEventRecord", "hipGetLastError",
         "hipStreamWaitEvent", "hipExtLaunchKernel:sum:512:9", "hipEventRecord", "hipStreamWaitEvent",
         "hipLaunchKernel:pack:96:7", "hipMemcpyAsync"]


def write(d, calls, tid=100, t0=1000, stream_base=0):
    os.makedirs(d)
    api = ['"Domain","Function","Process_Id","Thread_Id","Correlation_Id","Start_Timestamp","End_Timestamp"']
    ker = ['"Kind","Queue_Id","Stream_Id","Kernel_Name","Correlation_Id","Workgroup_Size_X","Grid_Size_X","Grid_Size_Y",'
           '"Grid_Size_Z"']
    for i, c in enumerate(calls):
        name, *k = c.split(":")
        api.append('"HIP_RUNTIME_API","%s",1,%d,%d,%d,%d' % (name, tid, t0 + i, t0 + 10 * i, t0 + 10 * i + 5))
        if k:
            ker.append('"KERNEL_DISPATCH",1,%d,"%s",%d,256,%s,1,1' % (int(k[2]) + stream_base, k[0], t0 + i, k[1]))
    with open(os.path.join(d, "r0_hip_api_trace.csv"), "w") as f:
        f.write("\n".join(api) + "\n")
    with open(os.path.join(d, "r0_kernel_trace.csv"), "w") as f:
        f.write("\n".join(ker) + "\n")
    return str(d)


def run(old, new):
    r = subprocess.run([sys.executable, TOOL, old, new], capture_output=True, text=True)
    return r.returncode, r.stdout


def test_same_operations_under_other_ids_are_equal(tmp_path):
    rc, out = run(write(tmp_path / "a", CALLS), write(tmp_path / "b", CALLS, tid=7, t0=50000, stream_base=30))
    assert rc == 0 and "PASS" in out, out
    assert "10 operations (3 kernel launches) equal" in out, out  # (hipGetLastError is not compared)


def test_differences_are_reported(tmp_path):
    old = write(tmp_path / "old", CALLS)
    moved = CALLS[:5] + [CALLS[6], CALLS[5]] + CALLS[7:]  # the wait after the launch it guarded
    other_stream = CALLS[:9] + ["hipLaunchKernel:pack:96:9"] + CALLS[10:]
    grid = CALLS[:2] + ["hipLaunchKernel:pack:128:7"] + CALLS[3:]
    for k, calls in enumerate((moved, other_stream, grid, CALLS[:-1])):
        rc, out = run(old, write(tmp_path / ("new%d" % k), calls))
        assert rc == 1 and "FAIL" in out and "first difference" in out, out
