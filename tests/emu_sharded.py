"""TEST INFRASTRUCTURE ONLY: the torch stand-in of ``ops.attn_temporal_sharded`` (the temporal attention of frame-sharded clips
with up to 128 key slots), next to tests/emu_ops.py, which stays as it is.  ``emu_ops.attn_temporal`` already takes a key mask of
any width and Tq <= T at any T, so the stand-in is that function; ``install`` puts both modules' stand-ins into
``mofa_video_amd.ops``."""
import emu_ops


def attn_temporal_sharded(q, k, v, nclips, T, HW, heads, head_dim=64, scale=None, out=None, Tq=None, key_mask=None):
    """k / v rows (clip, slot t < T, pixel); q / out rows (clip, frame i < Tq, pixel); key_mask bit j = key slot j exists"""
    return emu_ops.attn_temporal(q, k, v, nclips, T, HW, heads, head_dim=head_dim, scale=scale, out=out, Tq=Tq, key_mask=key_mask)


NAMES = ["attn_temporal_sharded"]


def install(monkeypatch=None):
    """emu_ops.install plus this module's stand-in.  monkeypatch=None: plain setattr (spawned worker processes)"""
    from mofa_video_amd import ops
    emu_ops.install(monkeypatch)
    for n in NAMES:
        if monkeypatch is not None:
            monkeypatch.setattr(ops, n, globals()[n])
        else:
            setattr(ops, n, globals()[n])
