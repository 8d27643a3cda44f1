"""Host checks of the capacity policy (isaac_ros_apriltag_amd/csrc/growth.h): which list of a handle grows after a submission,
and to what size.  Only what the GPU suite cannot reach is here -- the hard limits, capacities given at creation, several
overflows in one submission, the candidate flag rewrite, the long-record divisor and failed allocations; growth on real content
is exercised by the *_grows_with_the_content tests of tests/test_gpu_parity.py."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

NONE, CLUSTERS, QUADS, CANDS, POINTS, HASH = range(6)          # GrowFamily
PTS, TABLE, CL, QD, CAND = 0x1, 0x2, 0x4, 0x8, 0x20           # AMDAT_FLAG_* and AT_FLAG_CANDS

# a default 1920 x 1080 handle: one point per pixel (two at most), N/32 pair-table slots (N/8 at most), 65 536 clusters,
# 16 384 quads and candidates
CAPS = dict(pcap=2073600, lcap=259200, hcap=65536, ccap=65536, qcap=16384, cand_cap=16384, lcap_div=8)
LIMITS = dict(pcap_hard=4147200, hcap_hard=262144, ccap_hard=262144, points=1, hash=1, clusters=1, quads=1)


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("growth") / "growth_policy_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(HERE, "aux_c", "growth_policy_driver.cpp"), "-o", exe])

    def run(cmd, frames=(), mask=0, **over):
        caps = {k: over.get(k, v) for k, v in CAPS.items()}
        lim = {k: int(over.get(k, v)) for k, v in LIMITS.items()}
        words = [cmd] + list(caps.values()) + list(lim.values())
        if cmd != "pending":
            words += [mask, len(frames)]
            for f in frames:
                words += [f.get("points", 0), f.get("clusters", 0), f.get("quads", 0), f.get("flags", 0), f.get("nlong", 0)]
        out = subprocess.run([exe], input=" ".join(map(str, words)) + "\n", capture_output=True, text=True, check=True).stdout
        head, flags, tried, switches = out.split("|")
        v = [int(x) for x in head.split()]
        return dict(family=v[0], caps=dict(zip(CAPS, v[1:8])), cands_as_quads=bool(v[8]), hash_next=bool(v[9]),
                    flags=[int(x) for x in flags.split()], tried=[int(x) for x in tried.split()],
                    switches=dict(zip(("points", "hash", "clusters", "quads"), (int(x) for x in switches.split()))))
    return run


def grown(r, **caps):
    """The plan's capacities are the handle's except for `caps`."""
    return r["caps"] == dict(CAPS, **caps)


def test_no_overflow_grows_nothing(policy):
    r = policy("plan", [dict(points=2000000, clusters=4000, quads=40)] * 3)
    assert r["family"] == NONE and grown(r) and not r["cands_as_quads"] and not r["hash_next"]


@pytest.mark.parametrize("case", [
    # (family, frame, handle, capacities after)
    (CLUSTERS, dict(flags=CL, clusters=70000), {}, dict(ccap=131072)),                       # next power of two that holds it
    (CLUSTERS, dict(flags=CL, clusters=250000), {}, dict(ccap=262144)),
    (CLUSTERS, dict(flags=CL, clusters=250000), dict(ccap_hard=100000), dict(ccap=100000)),  # clamped to ccap_hard
    (NONE, dict(flags=CL, clusters=250000), dict(ccap=100000, ccap_hard=100000), {}),        # at ccap_hard: reported
    (QUADS, dict(flags=QD, quads=20000), {}, dict(qcap=32768)),
    (QUADS, dict(flags=QD, quads=20000), dict(ccap=20000), dict(qcap=20000)),               # qcap <= ccap
    (NONE, dict(flags=QD, quads=30000), dict(ccap=20000, qcap=20000), {}),
    (CANDS, dict(flags=CAND), dict(ccap=30000), dict(cand_cap=30000)),                       # cand_cap <= ccap
    (POINTS, dict(flags=PTS, points=4000000), dict(pcap=3000000), dict(pcap=4147200, lcap=518400)),   # clamped to pcap_hard
    (NONE, dict(flags=PTS, points=5000000), dict(pcap=4147200), {}),
    (POINTS, dict(flags=TABLE), dict(hcap=196608), dict(hcap=262144)),                       # clamped to hcap_hard
    (NONE, dict(flags=TABLE), dict(hcap=262144), {}),
])
def test_growth_stops_at_the_hard_limits(policy, case):
    family, frame, handle, after = case
    r = policy("plan", [frame], **handle)
    want = dict(CAPS, **{k: v for k, v in handle.items() if k in CAPS})
    want.update(after)
    assert r["family"] == family and r["caps"] == want, r


def test_pair_table_crowding_grows_before_the_next_submission(policy):
    crowded = [dict(clusters=65536 // 4 + 1)]
    assert policy("plan", crowded)["hash_next"] and policy("plan", [dict(clusters=65536 // 4)])["hash_next"] is False
    assert not policy("plan", crowded, hcap=262144)["hash_next"] and not policy("plan", crowded, hash=0)["hash_next"]
    r = policy("pending")
    assert r["family"] == HASH and grown(r, hcap=131072)
    assert grown(policy("pending", hcap=196608), hcap=262144)                               # clamped to hcap_hard
    assert policy("pending", hcap=262144)["family"] == NONE and policy("pending", hash=0)["family"] == NONE


@pytest.mark.parametrize("switch,frame", [
    ("clusters", dict(flags=CL, clusters=70000)),
    ("quads", dict(flags=QD, quads=20000)),
    ("points", dict(flags=PTS, points=3000000)),
    ("points", dict(flags=PTS, points=1000000, nlong=300000)),                                # the long records follow max_points
    ("hash", dict(flags=TABLE)),
])
def test_capacities_given_at_creation_never_grow(policy, switch, frame):
    assert policy("plan", [frame])["family"] != NONE
    r = policy("plan", [frame], **{switch: 0})
    assert r["family"] == NONE and grown(r) and r["flags"] == [frame["flags"]]


def test_one_family_per_relaunch_in_a_fixed_order(policy):
    """Clusters, then quads, then candidates, then points, long records and pair table together -- also when the overflows are
    spread over the frames of the submission."""
    frames = [dict(flags=PTS | TABLE, points=3000000, nlong=300000), dict(flags=CAND), dict(flags=QD, quads=20000),
              dict(flags=CL, clusters=70000)]
    assert policy("plan", frames)["family"] == CLUSTERS
    assert policy("plan", frames, clusters=0)["family"] == QUADS
    r = policy("plan", frames, clusters=0, quads=0)
    assert r["family"] == CANDS and grown(r, cand_cap=32768) and not r["cands_as_quads"]
    r = policy("plan", frames, clusters=0, quads=0, cand_cap=65536)
    assert r["family"] == POINTS and grown(r, pcap=4147200, hcap=131072, lcap_div=4, lcap=1036800, cand_cap=65536)
    assert r["cands_as_quads"]
    # a list whose flag is up but whose counter fits (it did not overflow itself) does not grow
    assert policy("plan", [dict(flags=CL, clusters=60000), dict(flags=QD, quads=16000)])["family"] == NONE


def test_candidate_overflow_that_cannot_grow_reports_a_quad_overflow(policy):
    frames = [dict(flags=CAND | TABLE), dict(flags=TABLE), dict(flags=CAND | QD, quads=10)]
    r = policy("plan", frames, cand_cap=65536, hash=0)
    assert r["family"] == NONE and r["cands_as_quads"] and r["flags"] == [QD | TABLE, TABLE, QD]
    r = policy("plan", frames, hash=0)                                                       # the list grows: nothing rewritten
    assert r["family"] == CANDS and not r["cands_as_quads"] and r["flags"] == [CAND | TABLE, TABLE, CAND | QD]


@pytest.mark.parametrize("nlong,points,div,pcap", [
    (300000, 1000000, 4, 2073600),       # a quarter of the point capacity holds it
    (600000, 1000000, 2, 2073600),       # half
    (3000000, 1000000, 1, 2073600),      # all of it (the divisor stops at 1)
    (600000, 2100000, 4, 4147200),       # the points overflowed too: a share of the doubled capacity
])
def test_long_record_divisor_halves_until_the_list_holds_the_frame(policy, nlong, points, div, pcap):
    # (the fullest frame decides; the points overflowed where the staging words did not fit or the long list did not either)
    r = policy("plan", [dict(flags=PTS, points=points, nlong=nlong), dict(flags=PTS, points=10, nlong=259201)])
    assert r["family"] == POINTS and grown(r, lcap_div=div, pcap=pcap, lcap=pcap // div)
    r = policy("plan", [dict(flags=PTS, points=1000000, nlong=3000000)], lcap_div=1, lcap=2073600)
    assert r["family"] == NONE                                                               # nothing left to halve


def test_points_flag_with_both_counters_within_capacity_grows_the_points(policy):
    """The points flag with neither counter above its list: not the long records (nlong fits), so the staging words."""
    r = policy("plan", [dict(flags=PTS, points=1000000, nlong=100000)])
    assert r["family"] == POINTS and grown(r, pcap=4147200, lcap=518400)


def test_long_capacity_has_a_floor(policy):
    r = policy("plan", [dict(flags=PTS, points=20000)], pcap=16000, lcap=4096, pcap_hard=32000)
    assert r["caps"]["pcap"] == 32000 and r["caps"]["lcap"] == 4096                          # (an eighth would be 4000)


def test_a_failed_allocation_gives_up_its_family_and_tries_the_next(policy):
    frames = [dict(flags=CL | CAND, clusters=70000), dict(flags=PTS, points=3000000)]
    # the candidate list has no switch: skipped for the rest of the round, its overflow reported, the points still grow
    r = policy("round", frames, mask=1 << CANDS, clusters=0)
    assert r["tried"] == [CANDS, POINTS] and r["family"] == POINTS and r["cands_as_quads"] and r["flags"] == [CL | QD, PTS]
    assert r["switches"] == dict(points=1, hash=1, clusters=0, quads=1)
    r = policy("round", frames, mask=(1 << CLUSTERS) | (1 << CANDS) | (1 << POINTS))
    assert r["tried"] == [CLUSTERS, CANDS, POINTS] and r["family"] == NONE and r["cands_as_quads"]
    assert r["switches"] == dict(points=0, hash=0, clusters=0, quads=1) and not r["hash_next"]
    r = policy("round", frames, mask=1 << CLUSTERS)
    assert r["tried"] == [CLUSTERS, CANDS] and r["family"] == CANDS and r["switches"]["clusters"] == 0
    r = policy("round", [dict(flags=QD, quads=20000)], mask=1 << QUADS)
    assert r["tried"] == [QUADS] and r["family"] == NONE and r["switches"]["quads"] == 0
