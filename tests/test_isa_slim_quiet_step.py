"""Code generation of the two sparse headline builds of ``k_rollout_lane`` after the quiet step was slimmed (CPU: hipcc
cross-compiles gfx950 to assembly here; the compile line is that of ``test_isa_invariants.py``).

The agents' wavefronts of these builds no longer run the select tree for the predicted value (it is read from the
table behind the row gather), the episode accounting or the schedule loads (both moved to the helper wavefronts); see
``csrc/qe_rollout_lane.h``, header comment, and DESIGN sections 4.3 and 9.  What the listing must show for it:

* nothing spills (``ScratchSize == 0``);
* no more VGPRs than the parent commit's build of the same symbol.  Measured at the parent with these flags: 116 for
  the plain build (the figure the change was proposed with) and 125 for the build with the delta log;
* the instruction behind a step barrier is not a full vector-memory wait (the cell load joins the row gather across
  the barrier: ``vmcnt(NLOAD + 1)``);
* the kernel function holds fewer instructions than the parent commit's: 2 706 (plain) and 2 964 (delta log) there,
  counted the same way -- lines of the function body that are neither labels, comments nor directives.  A fixed fact
  of the parent, not a target.
"""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dist_classicrl_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# name -> (symbol pattern, instructions at the parent, VGPRs at the parent)
SLIM_KERNELS = {
    "headline, sparse build": ("k_rollout_laneIfNS_7HashEnvELi4ELi128ELb0ELi1ELb1ELb1ELb1", 2706, 116),
    "headline, sparse build with the delta log": ("k_rollout_laneIfNS_7HashEnvELi4ELi128ELb0ELi2ELb1ELb1ELb1", 2964, 125),
}


@pytest.fixture(scope="module")
def lane_asm(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa_slim") / "lane.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-pass-failed",
           "-DQE_INST_T=float", "-DQE_INST_ENV=HashEnv", "-S", "--cuda-device-only", str(CSRC / "qe_inst_lane.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return out.read_text().split("\n")


def _kernel(lines, pattern):
    start = next(i for i, l in enumerate(lines) if pattern in l.split(":")[0] and ":" in l and not l.startswith(("\t", ".", ";", " ")))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    meta_end = next(i for i in range(end, len(lines)) if "; Occupancy" in lines[i])
    meta = {}
    for l in lines[end:meta_end + 1]:
        m = re.search(r"; (NumVgprs|ScratchSize|Occupancy): (\d+)", l)
        if m:
            meta[m.group(1)] = int(m.group(2))
    return lines[start + 1:end], meta


def _instructions(body):
    return [l.strip() for l in body if l.startswith("\t") and l.strip() and not l.strip().startswith((";", "."))]


@pytest.mark.parametrize("name", list(SLIM_KERNELS))
def test_no_spill_and_no_more_registers_than_the_parent(lane_asm, name):
    pattern, _, parent_vgprs = SLIM_KERNELS[name]
    _body, meta = _kernel(lane_asm, pattern)
    assert meta["ScratchSize"] == 0, meta
    assert meta["NumVgprs"] <= parent_vgprs, meta


@pytest.mark.parametrize("name", list(SLIM_KERNELS))
def test_no_full_vector_memory_wait_behind_a_step_barrier(lane_asm, name):
    body, _meta = _kernel(lane_asm, SLIM_KERNELS[name][0])
    barriers = 0
    for i, l in enumerate(body):
        # the step barriers are inline assembly: ;;#ASMSTART / s_waitcnt ... / s_barrier / ;;#ASMEND
        if l.strip() == "s_barrier" and "#ASMSTART" in body[i - 2]:
            barriers += 1
            j = i + 1
            while not body[j].strip() or body[j].strip().startswith(";"):
                j += 1
            assert not re.match(r"s_waitcnt vmcnt\(0\)", body[j].strip()), (
                f"{name}: `{body[j].strip()}` right behind the barrier at line {i} of the kernel")
    assert barriers >= 1
    # the loop's step barrier leaves the row gather AND the cell load in flight
    nload = 4
    assert any(re.match(rf"s_waitcnt vmcnt\({nload + 1}\) lgkmcnt\(0\)", l.strip()) for l in body)


@pytest.mark.parametrize("name", list(SLIM_KERNELS))
def test_fewer_instructions_than_the_parent_build(lane_asm, name):
    pattern, parent_count, _ = SLIM_KERNELS[name]
    body, _meta = _kernel(lane_asm, pattern)
    count = len(_instructions(body))
    print(f"{name}: {count} instructions (parent {parent_count})")
    assert count < parent_count
