"""GPU: raftq_node with RAFTQ_NODE_BEAT_DEVICE=1 -- every tick of a turn is raftq_tick_frames, the heartbeat round is built on the
device and queued ahead of everything else the turn sends.  The same scripted cluster is run with the switch off and on: the
commit channels and the WAL must be byte for byte the same, per (sender, addressee, group) the sequence of frames must be the host
path's -- and since a tick's heartbeats are a turn's first sends on the host path too, so must every polled stream as a whole."""
import collections

import numpy as np
import pytest

from tests import test_node_gpu as T

pytestmark = pytest.mark.gpu

MSG_HEARTBEAT = 8


@pytest.fixture()
def Cluster(gpu_engine_cls):
    from raftsql_amd.node import Cluster as C

    return C


def _per_group(frames):
    """[(sender, addressee, blob)] -> ({(sender, addressee, group): [frame bytes, in order]}, number of MsgHeartbeat frames)"""
    from oracle import pywire as W

    seq, beats = collections.defaultdict(list), 0
    for a, b, blob in frames:
        buf = np.frombuffer(blob, np.uint8)
        off, pos = [0], 0
        while pos < len(buf):
            pos += 8 + int.from_bytes(blob[pos:pos + 8], "big")
            off.append(pos)
        m, _, _ = W.wire_decode(buf, np.array(off, np.uint64))
        for i in range(len(m)):
            seq[(a, b, int(m["group"][i]))].append(blob[off[i]:off[i + 1]])
            beats += int(m["type"][i]) == MSG_HEARTBEAT
    return seq, beats


def _both(Cluster, monkeypatch, script, G, N, seed, beat_cap=None):
    def run(on):
        monkeypatch.setenv("RAFTQ_NODE_BEAT_DEVICE", "1" if on else "0")
        if beat_cap is not None:
            monkeypatch.setenv("RAFTQ_NODE_BEAT_CAP", str(beat_cap))
        c = Cluster(G, N, wal=True, seed=seed)
        try:
            seen = T._tap(c)
            c.start()
            script(c)
            chans = [[nd.drain(g) for g in range(G)] for nd in c.nodes]
            T.check_safety(c)
            built = sum(nd.stats()["msgs_built_on_device"] for nd in c.nodes)
            sent = sum(nd.stats()["msgs_sent"] for nd in c.nodes)
            return [(a, b, bytes(blob)) for a, b, blob in seen], [bytes(w) for w in c.wal], chans, built, sent
        finally:
            c.close()

    frames_h, wal_h, chans_h, built_h, sent_h = run(False)
    frames_d, wal_d, chans_d, built_d, sent_d = run(True)
    assert chans_h == chans_d, "commit channels"
    assert wal_h == wal_d, "WAL bytes"
    seq_h, beats_h = _per_group(frames_h)
    seq_d, beats_d = _per_group(frames_d)
    assert seq_h.keys() == seq_d.keys()
    for key in seq_h:
        assert seq_h[key] == seq_d[key], ("sender, addressee, group", key)
    assert frames_h == frames_d, "a polled stream differs as a whole"
    assert sent_h == sent_d and beats_h == beats_d and beats_d > 0
    return beats_d, built_d - built_h


def _election_round_trip(c):
    """elect, replicate, tick on (heartbeats), then another node campaigns for half of the groups: leadership moves, the old
    leaders' heartbeats stop and the new ones' start; more proposals and ticks under the new leaders"""
    G, N = c.G, len(c.nodes)
    T.elect(c)
    lead = c.leaders().copy()
    for wave in range(3):
        for g in range(G):
            c.nodes[int(lead[g])].propose(g, b"INSERT INTO t (v) VALUES (%d) -- g%d" % (wave, g))
        c.step()
    c.settle()
    c.run(4)
    moved = [g for g in range(G) if g % 2 == 0]
    by_node = collections.defaultdict(list)
    for g in moved:
        by_node[(int(lead[g]) + 1) % N].append(g)
    for p, gs in by_node.items():
        c.nodes[p].campaign(gs)
    c.run(3, tick=False)
    c.settle()
    T.elect(c)
    lead2 = c.leaders().copy()
    assert sum(int(lead2[g]) != int(lead[g]) for g in moved) >= len(moved) // 2, "leadership was meant to move"
    for wave in range(2):
        for g in range(G):
            c.nodes[int(lead2[g])].propose(g, b"UPDATE t SET v = %d -- g%d" % (wave, g))
        c.step()
    c.settle()
    c.run(5)
    c.settle()


def _partition_and_heal(c):
    """tests/test_node_gpu.py::test_partitioned_leader_cannot_commit_and_rejoins' script"""
    N = len(c.nodes)
    T.elect(c)
    g = 0
    old = int(c.leaders()[g])
    c.nodes[old].propose(g, b"a")
    c.settle()
    for q in range(N):
        if q != old:
            c.cut.add((old, q))
    c.nodes[old].propose(g, b"lost")  # reaches nobody
    c.run(3)
    l2 = []
    for _ in range(400):
        c.step()
        l2 = [p for p in range(N) if p != old and c.nodes[p].status(g).role == 2]
        if l2:
            break
    assert l2, "majority side elected no leader"
    c.nodes[l2[0]].propose(g, b"b")
    c.settle()
    c.run(2)
    c.settle()
    c.cut.clear()
    c.run(6)
    c.settle()
    assert c.nodes[old].status(g).role == 0
    assert b"lost" not in [d for _, d in c.nodes[old].log(g)]


def test_election_round_trip_is_the_host_paths(Cluster, monkeypatch):
    beats, built = _both(Cluster, monkeypatch, _election_round_trip, G=24, N=3, seed=11)
    assert built == beats, "every heartbeat of the run was meant to be built on the device"


def test_partition_and_heal_is_the_host_paths(Cluster, monkeypatch):
    beats, built = _both(Cluster, monkeypatch, _partition_and_heal, G=4, N=5, seed=3)
    assert built == beats


def test_groups_beyond_beat_cap_get_the_hosts_heartbeats(Cluster, monkeypatch):
    """RAFTQ_NODE_BEAT_CAP=3: a node that leads more than three groups builds the others' heartbeats on the host, as before"""
    beats, built = _both(Cluster, monkeypatch, _election_round_trip, G=24, N=3, seed=11, beat_cap=3)
    assert 0 < built < beats
