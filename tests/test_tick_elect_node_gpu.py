"""GPU: raftq_node with RAFTQ_NODE_ELECT_DEVICE=1 -- every tick of a turn is raftq_tick_elect_frames: the groups whose election timers
fired campaign on the device, their MsgVotes are queued directly behind the tick's heartbeats and no local MsgHup is raised.  The
same scripted cluster is run with the switch off and on (one tick per turn): the commit channels and the WAL must be byte for byte
the same, per (sender, addressee, group) the sequence of frames must be the host path's, and -- no raftq_node_campaign is pending
in a ticking turn of these scripts, RAFTQ_NODE_RESPOND_DEVICE is off -- so must every polled stream as a whole.  What the device
is expected to have built is counted in the HOST run's streams: the MsgVote frames its ticking turns sent."""
import collections

import numpy as np
import pytest

from tests import test_node_gpu as T
from tests import test_tick_frames_node_gpu as TN

pytestmark = pytest.mark.gpu

MSG_VOTE = 5


@pytest.fixture()
def Cluster(gpu_engine_cls):
    from raftsql_amd.node import Cluster as C

    return C


def _tap(c):
    """T._tap, with the step each poll belongs to: [(sender, addressee, blob, step number, the step ticked)]"""
    seen, at = [], {"step": 0, "tick": False}
    for p, nd in enumerate(c.nodes):
        orig = nd.poll

        def poll(q, _orig=orig, _p=p):
            b = _orig(q)
            if b:
                seen.append((_p, q, bytes(b), at["step"], at["tick"]))
            return b

        nd.poll = poll
    step = c.step

    def counted(tick=True):
        at["step"] += 1
        at["tick"] = bool(tick)
        return step(tick)

    c.step = counted
    return seen


def _timer_votes(frames, n_peers, cap):
    """the MsgVote frames the ticking turns sent, counting per (sender, step) only the first `cap` campaigning groups (ascending)"""
    from oracle import pywire as W

    groups = collections.defaultdict(set)
    for a, b, blob, step, tick in frames:
        if not tick:
            continue
        buf = np.frombuffer(blob, np.uint8)
        off, pos = [0], 0
        while pos < len(buf):
            pos += 8 + int.from_bytes(blob[pos:pos + 8], "big")
            off.append(pos)
        m, _, _ = W.wire_decode(buf, np.array(off, np.uint64))
        for g in m["group"][m["type"] == MSG_VOTE]:
            groups[(a, step)].add(int(g))
    return sum(min(len(gs), cap) for gs in groups.values()) * (n_peers - 1)


def _both(Cluster, monkeypatch, script, G, N, seed, elect_cap=None, beat_device=False):
    def run(on):
        monkeypatch.setenv("RAFTQ_NODE_ELECT_DEVICE", "1" if on else "0")
        monkeypatch.setenv("RAFTQ_NODE_BEAT_DEVICE", "1" if beat_device else "0")
        if elect_cap is not None:
            monkeypatch.setenv("RAFTQ_NODE_ELECT_CAP", str(elect_cap))
        c = Cluster(G, N, wal=True, seed=seed)
        try:
            seen = _tap(c)
            c.start()
            gone = script(c) or {"built": 0, "sent": 0}  # (the counters of a node the script stopped)
            live = [nd for p, nd in enumerate(c.nodes) if p not in c.down]
            chans = [[nd.drain(g) for g in range(G)] for nd in live]
            T.check_safety(c)
            built = gone["built"] + sum(nd.stats()["msgs_built_on_device"] for nd in live)
            sent = gone["sent"] + sum(nd.stats()["msgs_sent"] for nd in live)
            return seen, [bytes(w) for w in c.wal], chans, built, sent
        finally:
            c.close()

    frames_h, wal_h, chans_h, built_h, sent_h = run(False)
    frames_d, wal_d, chans_d, built_d, sent_d = run(True)
    assert chans_h == chans_d, "commit channels"
    assert wal_h == wal_d, "WAL bytes"
    seq_h, _ = TN._per_group([f[:3] for f in frames_h])
    seq_d, _ = TN._per_group([f[:3] for f in frames_d])
    assert seq_h.keys() == seq_d.keys()
    for key in seq_h:
        assert seq_h[key] == seq_d[key], ("sender, addressee, group", key)
    assert frames_h == frames_d, "a polled stream differs as a whole"
    want = _timer_votes(frames_h, N, G if elect_cap is None else elect_cap)
    all_votes = _timer_votes(frames_h, N, G)
    print(f"msgs_sent {sent_h} / {sent_d}; built on the device {built_h} -> {built_d}; timer MsgVotes {all_votes}, inside the cap {want}")
    assert sent_h == sent_d
    assert built_d - built_h == want and want > 0
    return want, all_votes


def _cold_start(c):
    """a cold-start election by timers, then proposals"""
    T.elect(c)
    lead = c.leaders().copy()
    for wave in range(3):
        for g in range(c.G):
            c.nodes[int(lead[g])].propose(g, b"INSERT INTO t (v) VALUES (%d) -- g%d" % (wave, g))
        c.step()
    c.settle()
    c.run(4)
    c.settle()


def _failover(c):
    """one node comes to lead every group (raftq_node_campaign, in turns that do not tick) and goes down; the others' timers
    elect; proposals continue"""
    G = c.G
    T.elect(c)
    lead = c.leaders().copy()
    c.nodes[0].campaign([g for g in range(G) if int(lead[g]) != 0])
    c.run(3, tick=False)
    c.settle()
    assert (c.leaders() == 0).all(), "node 0 was meant to lead every group"
    for g in range(G):
        c.nodes[0].propose(g, b"INSERT INTO t (v) VALUES (0) -- g%d" % g)
    c.step()
    c.settle()
    st = c.nodes[0].stats()
    gone = {"built": st["msgs_built_on_device"], "sent": st["msgs_sent"]}
    c.stop(0)
    T.elect(c)
    lead2 = c.leaders().copy()
    assert (lead2 > 0).all()
    for wave in range(2):
        for g in range(G):
            c.nodes[int(lead2[g])].propose(g, b"UPDATE t SET v = %d -- g%d" % (wave, g))
        c.step()
    c.settle()
    c.run(3)
    c.settle()
    return gone


def test_cold_start_election_is_the_host_paths(Cluster, monkeypatch):
    want, votes = _both(Cluster, monkeypatch, _cold_start, G=24, N=3, seed=11)
    assert want == votes


def test_failover_is_the_host_paths(Cluster, monkeypatch):
    want, votes = _both(Cluster, monkeypatch, _failover, G=16, N=3, seed=5)
    assert want == votes


def test_partition_and_heal_is_the_host_paths(Cluster, monkeypatch):
    want, votes = _both(Cluster, monkeypatch, TN._partition_and_heal, G=4, N=5, seed=3)
    assert want == votes


def test_groups_beyond_elect_cap_go_through_step(Cluster, monkeypatch):
    """RAFTQ_NODE_ELECT_CAP=3: of the timers that fire on one tick the first three campaign on the device, the rest as before"""
    want, votes = _both(Cluster, monkeypatch, _cold_start, G=24, N=3, seed=11, elect_cap=3)
    assert 0 < want < votes


def test_with_the_heartbeats_on_the_device_too(Cluster, monkeypatch):
    """RAFTQ_NODE_BEAT_DEVICE=1 in both runs: a tick's heartbeats and votes are one call's two sections"""
    want, votes = _both(Cluster, monkeypatch, _failover, G=16, N=3, seed=5, beat_device=True)
    assert want == votes
    want, votes = _both(Cluster, monkeypatch, _cold_start, G=24, N=3, seed=11, elect_cap=3, beat_device=True)
    assert 0 < want < votes
