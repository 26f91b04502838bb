"""Host-side mirror of the reference's nova-snark backend glue (vimz/src/nova_snark_backend/{input,folding}.rs):
same function names, argument meaning and error behaviour, driving the GPU through the C ABI.

    prepare_input   (input.rs:25-40)    VIMzInput -> per-step inputs + z0
    prepare_folding (folding.rs:20-25)  load_r1cs + create_public_params -> (circuit, FoldingParams)
    fold_input      (folding.rs:27-43)  create_recursive_circuit -> FoldingProof
    verify_folded_proof (folding.rs:45-56)
    compress_proof / verify_compressed_proof (mod.rs:52-67)  CompressedSNARK::{setup, prove, verify}
"""
import time

import numpy as np

from . import _lib
from .circuit import Circuit, default_shape

DEMO_STEPS = 10  # vimz/src/lib.rs:9
AUGMENTED_ROOM = 8192   # wires / constraints Nova's verifier circuit adds to a step circuit (vimz_ivc_create)
CYCLEFOLD_ROOM = 28672  # ... and Nova + CycleFold's main circuit F' (vimz_cf_create: 27.5 k — non-native folds of two CycleFold instances per step)
SECONDARY_KEY_LEN = 1 << 13   # generators of the secondary (Grumpkin) key: the secondary circuit has 7.6 k wires / rows

# vimz/src/transformation.rs:93-123
ITERATION_COUNT = {"SD": 480, "HD": 720, "FHD": 1080, "4K": 2160, "8K": 4320}
ITERATION_COUNT_BLOCK = {"HD": 576}
RATIO_TO_LOWER = {"HD": (3, 2), "FHD": (3, 2), "4K": (2, 1), "8K": (2, 1)}


def ivc_initial_state(transformation, inp):
    """Transformation::ivc_initial_state (vimz/src/transformation.rs:25-40)."""
    if transformation in ("blur", "sharpness"):
        return [0, 0, 0, 0]
    if transformation in ("brightness", "contrast"):
        return [0, 0, int(inp["factor"])]
    if transformation == "crop":
        return [0, 0, int(inp["info"])]
    if transformation in ("grayscale", "redact", "resize"):
        return [0, 0]
    if transformation == "hash":
        return [0]
    raise ValueError(transformation)


def iteration_count(transformation, resolution):
    if transformation == "redact":
        return ITERATION_COUNT_BLOCK[resolution]
    if transformation == "resize":
        return ITERATION_COUNT[resolution] // RATIO_TO_LOWER[resolution][0]
    return ITERATION_COUNT[resolution]


def prepare_step_input(step, transformation, inp, resolution):
    """prepare_step_input (input.rs:57-96): flattened private inputs of one step as (n, 4) limbs."""
    o, t = inp["original"], inp.get("transformed")
    if transformation in ("brightness", "contrast", "grayscale"):
        return np.concatenate([o[step], t[step]])
    if transformation in ("blur", "sharpness"):
        return np.concatenate([o[step:step + 3].reshape(-1, 4), t[step]])
    if transformation in ("crop", "hash"):
        return o[step]
    if transformation == "redact":
        ind = np.array([[int(inp["redact"][step]), 0, 0, 0]], dtype=np.uint64)
        return np.concatenate([o[step], ind])
    if transformation == "resize":
        a, b = RATIO_TO_LOWER[resolution]
        return np.concatenate([o[step * a:(step + 1) * a].reshape(-1, 4), t[step * b:(step + 1) * b].reshape(-1, 4)])
    raise ValueError(transformation)


def prepare_input(transformation, inp, resolution="HD", demo=False):
    """prepare_input (input.rs:25-40): returns (ivc_step_inputs (steps, n_priv, 4), initial_state)."""
    n = iteration_count(transformation, resolution)
    if demo:
        n = min(n, DEMO_STEPS)
    steps = np.stack([prepare_step_input(i, transformation, inp, resolution) for i in range(n)])
    return steps, ivc_initial_state(transformation, inp)


class FoldingParams:
    """The analogue of nova-snark's PublicParams: R1CS shape + both commitment keys (BN254 G1 for the primary circuit, Grumpkin for
    the secondary), resident on one GPU."""

    def __init__(self, ctx, circuit, ck, keygen_seconds, ck_secondary=None, kzg_vk=None, powers=None, verify_powers=False):
        self.ctx, self.circuit, self.ck, self.keygen_seconds, self.ck_secondary = ctx, circuit, ck, keygen_seconds, ck_secondary
        self.kzg_vk = kzg_vk      # backend "sonobe": [tau]G2 of the KZG SRS `ck` is (the decider's verifier needs it)
        self.verify_powers = bool(verify_powers)      # the decider judges the prefix of the string it reads (hip.verify_powers) before its set-up
        self.powers = powers      # ... or the powers-of-tau string `ck` was taken from: hip.Decider(prover, powers=params.powers) derives its key from the same

    def decider(self, prover, light=False):
        """The decider over `prover` (a CycleFoldIVC made with these keys): from the string when the keys came from one, else by a trapdoor drawn here."""
        from . import hip
        return hip.Decider(prover, powers=self.powers, light=light, verify_powers=self.verify_powers) if self.powers is not None else hip.Decider(prover, kzg_vk=self.kzg_vk, light=light)

    def secondary_key(self):
        if self.ck_secondary is None:
            self.ck_secondary = self.ctx.bases_generate(_lib.CURVE_GRUMPKIN, SECONDARY_KEY_LEN, b"ck-secondary")
        return self.ck_secondary

    def free(self):
        if self.ck_secondary is not None:
            self.ck_secondary.free()
            self.ck_secondary = None
        self.ck.free()


def _refuse_powers_without_kzg(powers, sonobe):
    if powers is not None and not sonobe:
        raise _lib.VimzError(_lib.ERR_INVALID, "prepare_folding: powers= is for the Sonobe backend (a KZG SRS); the nova-snark backend's key has no tau")


def prepare_folding(ctx, transformation, resolution="HD", ck_label=b"ck", window_tables=15, backend="nova-snark", powers=None, verify_powers=False):
    """prepare_folding (folding.rs:20-25): build the step circuit and derive the commitment key on the GPU.
    window_tables: 13..16 = window tables T_j[i] = 2^(c j)·P_i of the key in HBM with ONE bucket set shared by all windows
    (vimz_bases_precompute; default 15: 17 x the key = 0.7 GB at HD, 17 digits per scalar instead of 24 — the large MSM of a step
    1.10 -> 0.84 ms alone, the three-segment bench 964 -> 1095 steps/s, profiles/r04_msm_phases_tables.txt); 11 = tables with the usual
    per-window buckets (no Horner on the host); 0 = none.
    backend: "nova-snark" (vimz/src/nova_snark_backend) or "sonobe" (vimz/src/sonobe_backend: Nova + CycleFold, fold_input(mode="cyclefold"));
    the reference's two backends size their keys the same way (for the augmented circuit); Sonobe's is a KZG SRS (`KZG::setup` inside
    `prepare_folding`, vimz/src/sonobe_backend/folding.rs:36-48): powers of a tau drawn from the OS's randomness and forgotten
    (vimz_kzg_setup), whose [tau]G2 is kept in FoldingParams.kzg_vk for the decider's verifier.
    powers (backend "sonobe" only): iden3.read_ptau's dictionary — the SRS is then the string's first n points (hip.kzg_from_powers: no tau is drawn), and
    FoldingParams.decider derives the decider's key from the same string (hip.Decider(powers=)).  verify_powers=True: the string's prefix each of the two reads is
    judged first (hip.verify_powers); a refused string raises VimzError(ERR_INVALID).  Off by default."""
    _refuse_powers_without_kzg(powers, backend == "sonobe")
    t0 = time.time()
    circuit = Circuit(transformation, *default_shape(transformation, resolution))
    # next power of two, as nova-snark sizes ck — of the AUGMENTED circuit: the verifier circuit adds 7.7 k wires / rows
    n = 1 << (max(circuit.n_wires, circuit.n_constraints) + (CYCLEFOLD_ROOM if backend == "sonobe" else AUGMENTED_ROOM) - 1).bit_length()
    kzg_vk = None
    if backend == "sonobe":
        from . import hip
        ck, kzg_vk = hip.kzg_setup(ctx, n) if powers is None else hip.kzg_from_powers(ctx, powers, n, verify_powers=verify_powers)
    else:
        ck = ctx.bases_generate(_lib.CURVE_BN254_G1, n, ck_label)
    if window_tables:
        ck.precompute(16 if window_tables is True else int(window_tables))
    return circuit, FoldingParams(ctx, circuit, ck, time.time() - t0, kzg_vk=kzg_vk, powers=powers, verify_powers=verify_powers and powers is not None)


def prepare_folding_overlapped(device, segments, transformation, resolution="HD", window_tables=15, backend="nova-snark", mode="ivc", batch=0, ctxs=None, powers=None, verify_powers=False):
    """prepare_folding for a proof made as `segments` concurrent row segments, with its parts side by side instead of one after another
    (once the fold takes 0.6 s the set-up is the largest span of an HD run).  What depends on what:
        contexts (HIP runtime, streams)      — nothing; one thread each
        step circuit (host builder, 0.09 s)   — nothing: runs under the contexts' creation
        commitment key + window tables (GPU) — the circuit's size, context 0
        one prover per segment                — circuit, keys, its context: the verifier circuits' synthesis (host) and the device buffers of the
                                                segments' provers are made side by side (ctypes releases the GIL around every library call)
    Returns (ctxs, circuit, params, provers, seconds: {contexts_and_circuit, keys, provers, total}).  mode: "ivc" (hip.IVC), "cyclefold"
    (hip.CycleFoldIVC over a KZG SRS), "accumulator" (hip.Prover).  Sequential equivalent: prepare_folding + one prover per context.
    powers, verify_powers: as prepare_folding's (the Sonobe path only)."""
    import threading
    from . import hip
    _refuse_powers_without_kzg(powers, backend == "sonobe" or mode == "cyclefold")      # (before any context or thread exists)
    t_all = time.time()
    out, err = {}, []

    def guarded(fn):
        def run(*a):
            try:
                fn(*a)
            except BaseException as e:      # noqa: BLE001 (re-raised on the calling thread)
                err.append(e)
        return run

    own_ctxs = ctxs is None
    ctxs = [None] * segments if own_ctxs else list(ctxs)

    def make_ctx(k):
        ctxs[k] = hip.Context(device)

    circuit_built = threading.Event()

    def make_circuit():
        try:
            out["circuit"] = Circuit(transformation, *default_shape(transformation, resolution))
        finally:
            circuit_built.set()      # (the keys need its SIZE only: they are made while this thread goes on)
        if mode == "ivc":      # (the augmented circuits + their digests: 0.12 s of host work the segments' IVCs share — under the keys' generation)
            out["circuit"].prepare_ivc()

    # the step circuit and contexts 1.. on threads; context 0 here: the keys need only it and the circuit's size, and are made while the others still come up
    th_circ = threading.Thread(target=guarded(make_circuit))
    th_ctx = [threading.Thread(target=guarded(make_ctx), args=(k,)) for k in range(1, segments)] if own_ctxs else []
    for x in [th_circ] + th_ctx:
        x.start()
    if own_ctxs:
        guarded(make_ctx)(0)
    circuit_built.wait()
    if err or "circuit" not in out:
        th_circ.join()
        for x in th_ctx:
            x.join()
        raise err[0] if err else RuntimeError("the step circuit could not be built")
    circuit = out["circuit"]
    t_cc = time.time()
    sonobe = backend == "sonobe" or mode == "cyclefold"
    n = 1 << (max(circuit.n_wires, circuit.n_constraints) + (CYCLEFOLD_ROOM if sonobe else AUGMENTED_ROOM) - 1).bit_length()
    kzg_vk = None
    if sonobe:
        ck, kzg_vk = hip.kzg_setup(ctxs[0], n) if powers is None else hip.kzg_from_powers(ctxs[0], powers, n, verify_powers=verify_powers)
    else:
        ck = ctxs[0].bases_generate(_lib.CURVE_BN254_G1, n, b"ck")
    if window_tables:
        ck.precompute(16 if window_tables is True else int(window_tables))
    for x in th_ctx + [th_circ]:
        x.join()
    if err:
        raise err[0]
    params = FoldingParams(ctxs[0], circuit, ck, time.time() - t_cc, kzg_vk=kzg_vk, powers=powers, verify_powers=verify_powers and powers is not None)
    ck2 = params.secondary_key() if mode in ("ivc", "cyclefold") else None      # (mode "none": keys only, the caller makes its provers)
    t_keys = time.time()
    batch = batch or default_batch(circuit)
    provers = [None] * segments

    def make_prover(k):
        if mode == "none":
            return
        if mode == "ivc":
            provers[k] = hip.IVC(ctxs[k], circuit, ck, ck2, max_batch=batch)
        elif mode == "cyclefold":
            provers[k] = hip.CycleFoldIVC(ctxs[k], circuit, ck, ck2, max_batch=batch)
        else:
            provers[k] = hip.Prover(ctxs[k], circuit, ck, max_batch=batch)

    th = [threading.Thread(target=guarded(make_prover), args=(k,)) for k in range(segments)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    if err:
        raise err[0]
    t_end = time.time()
    return ctxs, circuit, params, provers, {"contexts_and_circuit": t_cc - t_all, "keys": t_keys - t_cc, "provers": t_end - t_keys, "total": t_end - t_all}


def default_batch(circuit):
    """Rows whose witnesses are generated together (and whose (A,B,C)·z and commitments the producer keeps ahead of the folds).  A batch costs one
    Poseidon-chain latency whatever its size, so wide circuits want large batches — and a batch buffer is rows x wires x 32 B, three provers per GPU.
    Round 5, measured as a trade-off (profiles/r05_batch_sweep.txt; three provers, steps/s over 256 / 128 / 128 rows and peak device memory):
        contrast HD   32: 1 160 / 13.8 GB    64: 1 181 / 21.4 GB    128: 1 219 / 35.6 GB
        contrast 4K   32:   673 / 31.4 GB    64:   693 / 52.8 GB    128:   704 / 97.6 GB
        resize 8K     32:   583 / 29.6 GB    64:   613 / 49.2 GB    128:   610 / 90.3 GB
    64 keeps every BASELINE configuration below 64 GB at a loss of at most 1.6 % against 128 (which was the default above 500 k wires until round 4:
    98-105 GB for three provers).  `--batch` / max_batch override it."""
    return 64


class FoldingProof:
    """FoldingProof (folding.rs:17): the RecursiveSNARK (mode "ivc": a vimz_ivc) or, in accumulator mode, the NIFS accumulator of
    the step circuit's own instances (a vimz_prover; mergeable across row segments, not a RecursiveSNARK)."""

    def __init__(self, prover, steps, z0, mode):
        self.prover, self.steps, self.z0, self.mode = prover, steps, z0, mode

    def instance(self):
        return self.prover.instance()

    def state(self):
        """The final IVC state z_n as integers."""
        if self.mode in ("ivc", "cyclefold"):
            return self.prover.state()[0]
        if self.mode in ("merged", "cyclefold-merged"):
            return self.prover.state()[1]
        return _limbs_to_ints(self.prover.instance()["z"])

    def close(self):
        """Release the proof and, for a merged proof, the segment provers and contexts fold_input created for it."""
        self.prover.close()
        for o in getattr(self, "_owned", []):
            o.close()
        self._owned = []


def _limbs_to_ints(a):
    return [sum(int(x[k]) << (64 * k) for k in range(4)) for x in np.asarray(a).reshape(-1, 4)]


def fold_input(params, ivc_step_inputs, initial_state, max_batch=None, prover=None, mode="ivc", segments=1):
    """fold_input (folding.rs:27-43): one RecursiveSNARK over all steps (mode "ivc", what the reference produces), or the NIFS
    accumulator (mode "accumulator").  Raises VimzError (the reference panics with "Failed to fold input").
    segments = S > 1 (mode "ivc"): the rows are proven as S contiguous segments folded CONCURRENTLY on this GPU (one IVC each, own
    context and streams) and merged into ONE proof object (vimz_ivc_merge; FoldingProof.mode == "merged") — a single chain leaves a
    quarter of an MI355X idle."""
    from .hip import IVC, Context, CycleFoldIVC, MergedProof, Prover
    if max_batch is None:
        max_batch = default_batch(params.circuit)
    if mode == "cyclefold" and prover is None and segments > 1 and len(ivc_step_inputs) >= segments:
        # S contiguous row segments folded concurrently (one CycleFold prover each, own context and streams) and merged into ONE object
        from .distributed import fold_concurrently, ivc_segments
        from .hip import CycleFoldMerged
        ctxs = [params.ctx] + [Context(params.ctx.device) for _ in range(segments - 1)]
        ck2 = params.secondary_key()
        cfs = [CycleFoldIVC(c, params.circuit, params.ck, ck2, max_batch=max_batch) for c in ctxs]
        try:
            from .distributed import fold_segments_merged
            merged = fold_segments_merged(cfs, ivc_step_inputs, initial_state, None, merged_cls=CycleFoldMerged)      # (start states staggered under the folds)
        except Exception:
            for o in cfs + ctxs[1:]:
                o.close()
            raise
        proof = FoldingProof(merged, len(ivc_step_inputs), list(initial_state), "cyclefold-merged")
        proof._owned = cfs + ctxs[1:]
        proof.verifier_key = cfs[0]
        return proof
    if mode == "cyclefold":        # the Sonobe backend's fold_input (vimz/src/sonobe_backend/folding.rs:52-66): Nova + CycleFold prove_step per row
        p = prover if prover is not None else CycleFoldIVC(params.ctx, params.circuit, params.ck, params.secondary_key(), max_batch=max_batch)
        p.reset(initial_state)
        p.fold(ivc_step_inputs)
        return FoldingProof(p, len(ivc_step_inputs), list(initial_state), "cyclefold")
    if prover is None and mode == "ivc" and segments > 1 and len(ivc_step_inputs) >= segments:
        from .distributed import fold_concurrently, ivc_segments
        ctxs = [params.ctx] + [Context(params.ctx.device) for _ in range(segments - 1)]
        ck2 = params.secondary_key()
        ivcs = [IVC(c, params.circuit, params.ck, ck2, max_batch=max_batch) for c in ctxs]
        try:
            segs = ivc_segments(ivcs, ivc_step_inputs, initial_state)
            for v, rows, z in segs:
                v.reset(z)
            fold_concurrently([(v, rows) for v, rows, z in segs])
            merged = MergedProof.of(ivcs)
        except Exception:
            for o in ivcs + ctxs[1:]:
                o.close()
            raise
        proof = FoldingProof(merged, len(ivc_step_inputs), list(initial_state), "merged")
        proof._owned = ivcs + ctxs[1:]          # (the first IVC is the merged proof's verifier key: released after it)
        proof.verifier_key = ivcs[0]
        return proof
    if prover is not None:
        p = prover
        mode = "ivc" if isinstance(prover, IVC) else "accumulator"
    elif mode == "ivc":
        p = IVC(params.ctx, params.circuit, params.ck, params.secondary_key(), max_batch=max_batch)
    else:
        p = Prover(params.ctx, params.circuit, params.ck, max_batch=max_batch)
    p.reset(initial_state)
    p.fold(ivc_step_inputs)
    return FoldingProof(p, len(ivc_step_inputs), list(initial_state), mode)


def verify_folded_proof(proof, params, num_steps, initial_state):
    """verify_folded_proof (folding.rs:45-56: RecursiveSNARK::verify(pp, num_steps, z0, [0])); raises like the reference's
    expect("Failed to verify folded proof")."""
    if proof.mode in ("ivc", "merged", "cyclefold", "cyclefold-merged"):      # (cyclefold: verify_folding, vimz/src/sonobe_backend/folding.rs:69-75)
        r = proof.prover.verify(num_steps, initial_state)
        if r != 0:
            raise _lib.VimzError(_lib.ERR_UNSAT, f"Failed to verify folded proof (flags {r:#x})")
        return
    inst = proof.prover.instance()
    if inst["steps"] != num_steps or list(initial_state) != list(proof.z0):
        raise _lib.VimzError(_lib.ERR_INVALID, "Failed to verify folded proof: step count / initial state mismatch")
    r = proof.prover.verify()
    if r != 0:
        raise _lib.VimzError(_lib.ERR_UNSAT, f"Failed to verify folded proof (flags {r:#x})")


COMPRESSED_MAGIC = {0x314E5343565A: "ivc", 0x31474D43565A: "merged", 0x314E534643565A: "cyclefold", 0x31474D4346565A: "cyclefold-merged"}


def compress_proof(params, proof):
    """CompressedSNARK::setup + prove (vimz/src/nova_snark_backend/mod.rs:52-59; spans "Prepare compression" / "Compress proof") for every proof
    fold_input returns but the accumulator: the Nova IVC ("ivc"), its merged segments ("merged"), the Nova + CycleFold chain ("cyclefold":
    vimz_cf_compress) and its merged segments ("cyclefold-merged": vimz_cf_merged_compress).  Returns (proof bytes, timings)."""
    if proof.mode not in ("ivc", "merged", "cyclefold", "cyclefold-merged"):
        raise _lib.VimzError(_lib.ERR_INVALID, "Failed to compress proof: only a RecursiveSNARK (mode \"ivc\", or merged segments) can be compressed")
    return proof.prover.compress()


def verify_compressed_proof(verifier_key, compressed, num_steps, initial_state):
    """compressed_proof.verify(&vk, num_steps, initial_state, secondary_initial_state) (mod.rs:63-67).  verifier_key: an IVC object
    created for the same step circuit and keys (e.g. proof.prover, or a fresh hip.IVC in another process); for the two Nova + CycleFold
    kinds a hip.CycleFoldIVC.  The blob's first word says which of the four kinds it is."""
    if isinstance(compressed, (bytes, bytearray, memoryview)):
        compressed = np.frombuffer(bytes(compressed), dtype=np.uint8)
    head = np.ascontiguousarray(compressed, dtype=np.uint8).reshape(-1)[:8]
    if head.size < 8:
        raise _lib.VimzError(_lib.ERR_INVALID, "Failed to verify proof: the blob is shorter than its header")
    from .hip import CycleFoldIVC, CycleFoldMerged, MergedProof
    kind = COMPRESSED_MAGIC.get(int(np.frombuffer(head.tobytes(), dtype=np.uint64)[0]))
    if kind is not None and kind.startswith("cyclefold") != isinstance(verifier_key, CycleFoldIVC):
        raise _lib.VimzError(_lib.ERR_INVALID, f"Failed to verify proof: a compressed \"{kind}\" proof needs a {'CycleFoldIVC' if kind.startswith('cyclefold') else 'IVC'} as its verifier key")
    if kind == "merged":      # a compressed MERGED proof (vimz_ivc_merged_compress)
        r = MergedProof.verify_compressed(verifier_key, compressed, num_steps, initial_state)
    elif kind == "cyclefold-merged":
        r = CycleFoldMerged.verify_compressed(verifier_key, compressed, num_steps, initial_state)
    else:
        r = verifier_key.verify_compressed(compressed, num_steps, initial_state)
    if r != 0:
        raise _lib.VimzError(_lib.ERR_UNSAT, f"Failed to verify proof (flags {r:#x})")


def verify_compressed_proofs(verifier_key, blobs, num_steps, initial_states, chunk=0, bisect=True, leaf=0, stats=None):
    """Many compressed proofs under one verifier key in one call (vimz_ivc_verify_compressed_batch / vimz_cf_verify_compressed_batch): the group equations of
    a chunk of proofs (0 = 32) are judged as one, on the GPU.  verifier_key: a hip.IVC for "ivc" / "merged" blobs, a hip.CycleFoldIVC for the two Nova +
    CycleFold kinds; the kinds of a family may be mixed, a blob of the other family gets the malformed bit.  Returns the flag words, one a proof — the word
    verify_compressed_proof's entry gives for that proof alone, 0 = accepted — and does not raise on a bad member.  A refused chunk is bisected: its equations
    are asked again of halves, down to refused subsets of `leaf` proofs (0 = 1), which the single verifier judges; bisect=False sends the chunk there whole.
    stats: a dict that receives hip.BATCH_STATS (chunks refused, subset equations, single verifications, members a subset equation accepted)."""
    return verifier_key.verify_compressed_batch(blobs, num_steps, initial_states, chunk, bisect=bisect, leaf=leaf, stats=stats)[0]


# ---- a proof's final state against its images (the Sonobe path's verify_final_state_arkworks, vimz/src/sonobe_backend/folding.rs:77-132) ----

def _gpu_hasher(ctx):
    from . import image_hasher

    def run(specs):
        return image_hasher.image_hashes(ctx, specs)
    return run


def _hash_specs(hasher, specs, ctx=None):
    """hasher: a callable specs -> [int] (tests inject the CPU oracle), a hip.Context, or None (the GPU: `ctx` if given, else a context on device 0
    for this call).  Every spec goes in ONE call: the source and the target of a proof are hashed together."""
    if callable(hasher) and not hasattr(hasher, "image_hash"):
        return hasher(specs)
    if hasher is not None:
        return _gpu_hasher(hasher)(specs)
    if ctx is not None:
        return _gpu_hasher(ctx)(specs)
    from .hip import Context
    with Context(0) as c:
        return _gpu_hasher(c)(specs)


def final_state_units(transformation, resolution="HD", demo=False):
    """(steps n, source units, target units) of a proof of `transformation`: n is its step count (DEMO_STEPS at most in demo mode), and it hashes
    n rows (blocks for redact) of each image into its final state — resize a·n source rows and b·n target rows (RATIO_TO_LOWER)."""
    n = iteration_count(transformation, resolution)
    if demo:
        n = min(n, DEMO_STEPS)
    if transformation == "resize":
        a, b = RATIO_TO_LOWER[resolution]
        return n, a * n, b * n
    return n, n, n


def expected_final_state(transformation, source, target, resolution="HD", demo=False, redact=None, hasher=None, ctx=None):
    """{index: value}: the entries of a proof's final state z_n that the images determine — z_n[0] the running hash of `source`, z_n[1] that of
    `target` (either may be None: not checked).  Images are arrays or paths (vimz_amd.image_hasher).
        hash              z[0] only: the transformation has no target
        blur / sharpness  z[0] is the hash of the UNPADDED source (the circuit hashes the middle of its three rows); z[2], z[3] are row bookkeeping
        resize            a·n source rows, b·n target rows, each image at its own width
        redact            40 x 40 blocks; the target's redacted blocks enter as PairHasher(acc, 0), not as the digest of a black block, so the
                          target needs `redact` (the input's flags)
        crop              the target is refused: the crop circuit's z[1] is not the hash of the cropped image (its decoder reads the offsets from
                          other bit fields than the input's `info` encodes and packs the R byte alone, SURVEY.md F6 — tests/test_image_hash_host.py
                          shows it on the oracle)
    hasher: None (the GPU, on `ctx` or a context of its own), a hip.Context, or a callable taking the request dicts of image_hasher.image_hashes."""
    if transformation not in ("blur", "brightness", "contrast", "crop", "grayscale", "hash", "redact", "resize", "sharpness"):
        raise ValueError(transformation)
    n, n_src, n_tgt = final_state_units(transformation, resolution, demo)
    mode = "blocks" if transformation == "redact" else "rows"
    specs, idx = [], []
    if source is not None:
        specs.append({"image": source, "mode": mode, "units": n_src})
        idx.append(0)
    if target is not None:
        if transformation == "hash":
            raise _lib.VimzError(_lib.ERR_INVALID, "A proof of `hash` determines no target image")
        if transformation == "crop":
            raise _lib.VimzError(_lib.ERR_INVALID, "Target image check is not supported for crop: the crop circuit's final state is not the hash of "
                                                    "the cropped image (SURVEY.md F6)")
        spec = {"image": target, "mode": mode, "units": n_tgt}
        if transformation == "redact":
            if redact is None:
                raise _lib.VimzError(_lib.ERR_INVALID, "redact: the target image's hash needs the input's redact flags (redact=)")
            flags = [int(v) for v in list(redact)[:n_tgt]]
            if len(flags) < n_tgt:
                raise _lib.VimzError(_lib.ERR_INVALID, f"redact: {len(flags)} redact flags for {n_tgt} blocks")
            spec["drop"] = flags
        specs.append(spec)
        idx.append(1)
    if not specs:
        return {}
    return dict(zip(idx, [int(v) for v in _hash_specs(hasher, specs, ctx)]))


def verify_final_state(proof_or_state, transformation, source_image=None, target_image=None, resolution="HD", demo=False, redact=None, hasher=None):
    """verify_final_state_arkworks (vimz/src/sonobe_backend/folding.rs:77-132): the final state of a proof against the images it claims to be about.
    proof_or_state: a FoldingProof of any mode (its step count must be the transformation's, as the reference asserts) or a plain z_n (e.g. the
    decider's public z_i).  Raises VimzError(ERR_UNSAT, "Source image hash does not match final state") or the Target equivalent."""
    ctx = None
    if isinstance(proof_or_state, FoldingProof):
        n = final_state_units(transformation, resolution, demo)[0]
        if proof_or_state.steps != n:
            raise _lib.VimzError(_lib.ERR_UNSAT, f"The proof folds {proof_or_state.steps} steps, {transformation} at {resolution} takes {n}")
        z = [int(v) for v in proof_or_state.state()]
        ctx = getattr(proof_or_state.prover, "ctx", None)
    else:
        z = [int(v) for v in proof_or_state]
    exp = expected_final_state(transformation, source_image, target_image, resolution, demo, redact, hasher, ctx)
    for i, who in ((0, "Source"), (1, "Target")):
        if i in exp and (i >= len(z) or z[i] != exp[i]):
            raise _lib.VimzError(_lib.ERR_UNSAT, f"{who} image hash does not match final state")
