"""The session every parser handle keeps (csrc/parser_host.hpp): one batch at a time, the entry checks, host inputs staged once, copy-out with
per-frame capacity status - the same cases over Paf, PoseProposal and PifPaf.  That the humans are the reference's is the business of
test_paf_gpu / test_ppn / test_pifpaf; here the paths of one handle are compared with each other, byte for byte.

Inputs: three frames at the generators' default map sizes from a fixed seed, people = (1, 3, 1).  REF_COUNTS are the humans per frame
that the reference's own code (oracle/_ref) finds in exactly these maps, for all three parsers - recorded once on the CPU; frame 1
is the frame with more than one human, frames 0 and 2 fit a capacity of one."""
import numpy as np
import pytest

from hyperpose_amd import synth

pytestmark = pytest.mark.gpu

B, SALT, PEOPLE, REF_COUNTS = 3, 41, (1, 3, 1), [1, 3, 1]


class _Paf:
    kind, tail_env = "paf", None

    @staticmethod
    def maps():
        conf, paf, _ = synth.paf_maps(synth.rng_for(1, salt=SALT), B, people=PEOPLE)
        return [conf, paf]

    @staticmethod
    def make(cap=128):
        from hyperpose_amd.parser import Paf
        return Paf(max_batch=B, cap_per_frame=cap)

    @staticmethod
    def host(p, m):
        return p.process_batch(m[0], m[1])

    @staticmethod
    def device(p, d, n, m):
        return p.process_batch_device(d[0], d[1], n, m[0].shape[1:], m[1].shape[1:])

    @staticmethod
    def enqueue(p, d, n, m, stream=None):
        p.enqueue(d[0], d[1], n, m[0].shape[1:], m[1].shape[1:], stream)


class _Ppn:
    kind, tail_env = "ppn", "HP_PPN_HOST_TAIL"

    @staticmethod
    def maps():
        return [np.ascontiguousarray(a) for a in synth.ppn_maps(synth.rng_for(3, salt=SALT), B, people=PEOPLE)]

    @staticmethod
    def make(cap=128):
        from hyperpose_amd.parser import PoseProposal
        return PoseProposal((384, 384), max_batch=B, cap_per_frame=cap)

    @staticmethod
    def host(p, m):
        return p.process_batch(m)

    @staticmethod
    def device(p, d, n, m):
        return p.process_batch(d, on_device=True, n=n, conf_shape=m[0].shape[1:], edge_shape=m[6].shape[1:])

    @staticmethod
    def enqueue(p, d, n, m, stream=None):
        p.enqueue(d, n, m[0].shape[1:], m[6].shape[1:], stream)


class _PifPaf:
    kind, tail_env = "pifpaf", "HP_PIFPAF_HOST_TAIL"

    @staticmethod
    def maps():
        return list(synth.pifpaf_maps(synth.rng_for(2, salt=SALT), B, people=PEOPLE))

    @staticmethod
    def make(cap=128):
        from hyperpose_amd.parser import PifPaf
        return PifPaf(385, 385, max_batch=B, cap_per_frame=cap)

    @staticmethod
    def host(p, m):
        return p.process_batch(m[0], m[1])

    @staticmethod
    def device(p, d, n, m):
        return p.process_batch(d[0], d[1], on_device=True, n=n, fh=m[1].shape[-2], fw=m[1].shape[-1])

    @staticmethod
    def enqueue(p, d, n, m, stream=None):
        p.enqueue(d[0], d[1], n, m[1].shape[-2], m[1].shape[-1], stream)


KINDS = {k.kind: k for k in (_Paf, _Ppn, _PifPaf)}
_shared = {}


def _case(hp, kind):
    """(adapter, host maps, device copies, the uncapped lists of the three frames) - made once per parser and left unchanged."""
    if kind not in _shared:
        K = KINDS[kind]
        m = K.maps()
        want = K.host(K.make(), m)
        assert [len(h) for h in want] == REF_COUNTS
        _shared[kind] = (K, m, [hp.DevBuf.from_numpy(a) for a in m], want)
    return _shared[kind]


def _same(got, want):
    return len(got) == len(want) and all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, want))


def _raw_collect(hp, K, p):
    """hp_<kind>_collect as the library answers it, past the Python class."""
    return getattr(hp.lib(), f"hp_{K.kind}_collect")(p._h, p._out, p.cap, p._n)


@pytest.mark.parametrize("kind", list(KINDS))
def test_collect_with_nothing_enqueued(hp, kind):
    K, m, d, want = _case(hp, kind)
    p = K.make()
    with pytest.raises(hp.HpError) as e:
        p.collect()
    assert e.value.code == hp.HP_ERR_STATE
    assert _same(K.host(p, m), want)


@pytest.mark.parametrize("kind", list(KINDS))
def test_second_enqueue_is_refused_and_the_first_batch_survives(hp, kind):
    K, m, d, want = _case(hp, kind)
    p = K.make()
    K.enqueue(p, d, B, m)
    with pytest.raises(hp.HpError) as e:
        K.enqueue(p, d, B, m)
    assert e.value.code == hp.HP_ERR_STATE
    assert _same(p.collect(), want)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", [0, B + 1])
def test_batch_size_out_of_range(hp, kind, n):
    K, m, d, want = _case(hp, kind)
    p = K.make()
    sized = [np.concatenate([a, a[:1]])[:n] for a in m]  # n frames of host input (the device buffers are refused before they are read)
    for call in (lambda: K.enqueue(p, d, n, m), lambda: K.device(p, d, n, m), lambda: K.host(p, sized)):
        with pytest.raises(hp.HpError) as e:
            call()
        assert e.value.code == hp.HP_ERR_CAPACITY
        assert _raw_collect(hp, K, p) == hp.HP_ERR_STATE  # nothing is pending
    assert _same(K.host(p, m), want)


@pytest.mark.parametrize("kind", list(KINDS))
def test_capacity_of_one(hp, kind):
    K, m, d, want = _case(hp, kind)
    p = K.make(cap=1)
    with pytest.raises(hp.HpError) as e:
        K.host(p, m)
    assert e.value.code == hp.HP_ERR_CAPACITY and "frame 1 " in str(e.value)
    assert list(p._n[:B]) == REF_COUNTS  # the true counts
    got = np.frombuffer(p._out, dtype=hp.HUMAN_DTYPE)
    for f in range(B):  # frame 1: the first of its three humans; frames 0 and 2 are complete
        assert got[f:f + 1].tobytes() == want[f][:1].tobytes(), f


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_way_in_gives_the_same_bytes(hp, kind):
    from hyperpose_amd.parser import Paf
    K, m, d, want = _case(hp, kind)
    p = K.make()
    assert _same(K.host(p, [a[:1] for a in m]), want[:1])  # the staging buffers are sized by this first, smallest call
    assert _same(K.host(p, m), want)
    assert _same(K.device(p, d, B, m), want)
    caller = Paf(max_batch=1)  # a stream that is not the parser's: another handle's
    K.enqueue(p, d, B, m, caller.stream)
    p.after(caller.stream)
    assert _same(p.collect(), want)


@pytest.mark.parametrize("kind", ["ppn", "pifpaf"])
def test_host_tail_gives_the_same_bytes(hp, monkeypatch, kind):
    K, m, d, want = _case(hp, kind)
    monkeypatch.setenv(K.tail_env, "1")
    p = K.make()
    monkeypatch.delenv(K.tail_env)
    assert _same(K.host(p, m), want)
    assert list(p.decode_flags(B)) == [-1] * B
    K.enqueue(p, d, B, m)
    assert _same(p.collect(), want)
