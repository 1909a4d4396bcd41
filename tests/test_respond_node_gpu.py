"""GPU: raftq_node with RAFTQ_NODE_RESPOND_DEVICE=1 -- the fused inbound round is raftq_step_frames_respond, the responses and
commit broadcasts of the round are built on the device and queued ahead of the turn's host-built frames.  Every node runs
with RAFTQ_NODE_RESPOND_CHECK=1: a set at-tail bit that is not true poisons the node.

What may differ from the host path is only the interleaving of different groups in a peer's stream (and the place of a tick's
heartbeats): per (batch, sender, addressee, group) the frames must be the host path's, the WAL and the commit channels
byte for byte the same."""
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


@pytest.fixture()
def respond_on(monkeypatch):
    monkeypatch.setenv("RAFTQ_NODE_RESPOND_DEVICE", "1")
    monkeypatch.setenv("RAFTQ_NODE_RESPOND_CHECK", "1")


def _per_group(frames):
    """[(sender, addressee, blob)] -> {(batch, sender, addressee, group): [frame bytes]}, heartbeats kept apart per
    (sender, addressee, group) -- the one kind whose place against a device-built answer the option moves"""
    from oracle import pywire as W

    seq, beats = collections.defaultdict(list), collections.Counter()
    for k, (a, b, blob) in enumerate(frames):
        buf = np.frombuffer(blob, np.uint8)
        off, pos = [0], 0
        while pos < len(buf):
            pos += 8 + int.from_bytes(blob[pos:pos + 8], "big")
            off.append(pos)
        m, _, _ = W.wire_decode(buf, np.array(off, np.uint64))
        for i in range(len(m)):
            fr = blob[off[i]:off[i + 1]]
            g = int(m["group"][i])
            if int(m["type"][i]) == MSG_HEARTBEAT:
                beats[(a, b, g, fr)] += 1
            else:
                seq[(k, a, b, g)].append(fr)
    return seq, beats


@pytest.mark.parametrize("N,per_turn,interleave", [(3, 1, False), (5, 3, False), (3, 3, True)])
def test_device_built_answers_are_the_hosts_per_group(Cluster, N, per_turn, interleave, monkeypatch):
    """test_device_built_msgapps_are_the_hosts_byte_for_byte's script with the option off and on"""
    G = 24

    def run(on):
        monkeypatch.setenv("RAFTQ_NODE_RESPOND_DEVICE", "1" if on else "0")
        monkeypatch.setenv("RAFTQ_NODE_RESPOND_CHECK", "1")
        c = Cluster(G, N, wal=True, seed=11)
        try:
            seen = T._tap(c)
            c.start()
            T.elect(c)
            lead = c.leaders().copy()
            built0 = sum(nd.stats()["msgs_built_on_device"] for nd in c.nodes)
            for wave in range(6):
                order = [(g, k) for g in range(G) for k in range(per_turn if g % 3 else 1)]
                if interleave:
                    order.sort(key=lambda gk: (gk[1], gk[0]))
                for g, k in order:
                    proposer = int(lead[g]) if (g + wave) % 4 else (int(lead[g]) + 1) % N
                    c.nodes[proposer].propose(g, b"INSERT INTO t (v) VALUES (%d) -- g%d w%d" % (k, g, wave))
                c.step()
            c.settle()
            c.run(2)
            c.settle()
            assert (c.leaders() == lead).all()
            chans = [[nd.drain(g) for g in range(G)] for nd in c.nodes]
            T.check_safety(c)
            built = sum(nd.stats()["msgs_built_on_device"] for nd in c.nodes) - built0
            return [(a, b, bytes(blob)) for a, b, blob in seen], [bytes(w) for w in c.wal], chans, built
        finally:
            c.close()

    frames_h, wal_h, chans_h, built_h = run(False)
    frames_d, wal_d, chans_d, built_d = run(True)
    assert chans_h == chans_d
    assert wal_h == wal_d
    assert [(a, b) for a, b, _ in frames_h] == [(a, b) for a, b, _ in frames_d]
    assert [len(x) for _, _, x in frames_h] == [len(x) for _, _, x in frames_d]
    seq_h, beats_h = _per_group(frames_h)
    seq_d, beats_d = _per_group(frames_d)
    assert beats_h == beats_d
    assert seq_h.keys() == seq_d.keys()
    for key in seq_h:
        assert seq_h[key] == seq_d[key], ("batch, sender, addressee, group", key)
    # the answers went through the device: every MsgAppResp of an append at the tail and every commit broadcast at least
    assert built_d - built_h > 6 * G


def test_new_db_with_answers_on_the_device(Cluster, respond_on):
    T.test_new_db_analog_three_nodes(Cluster)


def test_restart_with_answers_on_the_device(Cluster, respond_on):
    T.test_restart_db_analog(Cluster)


def test_partition_with_answers_on_the_device(Cluster, respond_on):
    T.test_partitioned_leader_cannot_commit_and_rejoins(Cluster)


@pytest.mark.parametrize("seed,from_wal", [(1, False), (2, False), (3, False), (4, True)])
def test_chaos_with_answers_on_the_device(Cluster, respond_on, seed, from_wal):
    T.test_chaos_safety_and_convergence(Cluster, seed, from_wal, False)
