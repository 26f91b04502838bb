"""Readers for circom's artefacts in the iden3 binary formats — `.r1cs` (constraints) and `.wtns` (one witness) — for ANY prime, in Python:
what `load_r1cs` / `generate_witness_from_bin` hand to nova-scotia (vimz/src/nova_snark_backend/folding.rs:22, :35-41), feeding the
seam-based accumulator (`vimz_amd.nifs`).  (The native reader `vimz_circuit_load_r1cs` serves the BN254 provers.)

Column order: circom numbers the wires [1 | public outputs | public inputs | private]; nova-snark's R1CSShape orders an assignment
z = [W (private wires) | u | X (public wires)] — `to_nova_columns` maps one onto the other the way nova-scotia's CircomCircuit does."""
import struct
import sys

import numpy as np


def _sections(data, magic):
    if data[:4] != magic:
        raise ValueError(f"not a {magic.decode()} file")
    _version, nsec = struct.unpack_from("<II", data, 4)
    pos, out = 12, {}
    for _ in range(nsec):
        t, size = struct.unpack_from("<IQ", data, pos)
        pos += 12
        out[t] = data[pos:pos + size]
        pos += size
    return out


def read_r1cs(data):
    """-> dict(prime, n_wires, n_pub_out, n_pub_in, n_prv, n_constraints, A, B, C) with A, B, C as (rows u32, wires u32, values (nnz, 4) u64
    canonical) triplets in circom's wire numbering."""
    sec = _sections(bytes(data), b"r1cs")
    hdr = sec[1]
    fs = struct.unpack_from("<I", hdr, 0)[0]
    if fs != 32:
        raise ValueError("only 32-byte field elements are supported")
    prime = int.from_bytes(hdr[4:36], "little")
    n_wires, n_pub_out, n_pub_in, n_prv, _n_labels, ncon = struct.unpack_from("<IIIIQI", hdr, 36)
    body, pos = sec[2], 0
    mats = [([], [], []) for _ in range(3)]
    for k in range(ncon):
        for rows, wires, vals in mats:
            n = struct.unpack_from("<I", body, pos)[0]
            pos += 4
            for _ in range(n):
                w = struct.unpack_from("<I", body, pos)[0]
                rows.append(k); wires.append(w); vals.append(body[pos + 4:pos + 36])
                pos += 36
    def pack(m):
        rows, wires, vals = m
        v = np.frombuffer(b"".join(vals), dtype=np.uint64).reshape(-1, 4).copy() if vals else np.zeros((0, 4), dtype=np.uint64)
        return np.asarray(rows, dtype=np.uint32), np.asarray(wires, dtype=np.uint32), v
    A, B, C = (pack(m) for m in mats)
    return {"prime": prime, "n_wires": n_wires, "n_pub_out": n_pub_out, "n_pub_in": n_pub_in, "n_prv": n_prv, "n_constraints": ncon, "A": A, "B": B, "C": C}


def read_wtns(data):
    """-> (prime, (n_wires, 4) uint64 canonical values in circom's wire order; wire 0 is the constant 1)."""
    sec = _sections(bytes(data), b"wtns")
    hdr = sec[1]
    fs = struct.unpack_from("<I", hdr, 0)[0]
    if fs != 32:
        raise ValueError("only 32-byte field elements are supported")
    prime = int.from_bytes(hdr[4:36], "little")
    n = struct.unpack_from("<I", hdr, 36)[0]
    return prime, np.frombuffer(sec[2], dtype=np.uint64).reshape(n, 4).copy()


BN254_Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
_PTAU_SECTIONS = ((2, "tau_g1", 64), (3, "tau_g2", 128), (4, "alpha_g1", 64), (5, "beta_g1", 64), (6, "beta_g2", 128))      # section, name, bytes per point


def read_ptau(data):
    """A powers-of-tau file (snarkjs's `.ptau` container, magic "ptau") -> dict(power, ceremony_power, tau_g1, tau_g2, alpha_g1, beta_g1, beta_g2): read-only
    uint64 views of `data` (no copy), one row per point, 4 words per coordinate, in the file's own (Montgomery) form.  Sections: 1 = n8, the prime, the power,
    the ceremony's power; 2 tau_g1 (2^(power+1) − 1 points), 3 tau_g2, 4 alpha_g1, 5 beta_g1 (2^power each), 6 beta_g2 (one).  Points are affine and
    uncompressed, every coordinate 32 bytes little-endian in Montgomery form, G2 as x.c0, x.c1, y.c0, y.c1.  UNPINNED: the layout is restated from snarkjs's
    published format and this reader has not yet read a real ceremony file.  ValueError for a truncated container, a missing section, a prime other than BN254's
    q and section lengths that do not match the power; the points themselves are not judged here."""
    data = bytes(data)
    try:
        sec = _sections(data, b"ptau")
    except struct.error:
        raise ValueError("ptau: the file ends inside its section table") from None
    pos = 12
    for _ in range(struct.unpack_from("<I", data, 8)[0]):      # (slices past the end come back short without a complaint)
        pos += 12 + struct.unpack_from("<Q", data, pos + 4)[0]
        if pos > len(data):
            raise ValueError("ptau: the file ends inside a section")
    hdr = sec.get(1)
    if hdr is None:
        raise ValueError("ptau: no header section")
    if len(hdr) < 4 or struct.unpack_from("<I", hdr, 0)[0] != 32:
        raise ValueError("ptau header: only 32-byte field elements are supported")
    if len(hdr) != 4 + 32 + 8:
        raise ValueError(f"ptau header: {len(hdr)} bytes, expected 44 (n8, the prime, the power, the ceremony's power)")
    if int.from_bytes(hdr[4:36], "little") != BN254_Q:
        raise ValueError("ptau header: the prime is not BN254's base field modulus")
    power, ceremony_power = struct.unpack_from("<II", hdr, 36)
    if not 1 <= power <= 26:
        raise ValueError("ptau header: power outside 1..26")
    n2 = 1 << power
    out = {"power": power, "ceremony_power": ceremony_power}
    for t, name, size in _PTAU_SECTIONS:
        points = {"tau_g1": 2 * n2 - 1, "beta_g2": 1}.get(name, n2)
        body = sec.get(t)
        if body is None:
            raise ValueError(f"ptau section {t} ({name}) is missing")
        if len(body) != points * size:
            raise ValueError(f"ptau section {t} ({name}): {len(body)} bytes, the power asks for {points * size}")
        out[name] = np.frombuffer(body, dtype="<u8").reshape(points, size // 8)
    return out


def write_ptau(powers):
    """read_ptau's dictionary -> the bytes of a `.ptau` container: the exact inverse of read_ptau (read_ptau(write_ptau(p)) holds p's words).  Writes version 1 and the
    sections 1–6 in their order and nothing else — no contribution section 7 and none of the Lagrange sections 12–15 of a file `prepare phase2` has been run on.  Rows
    are uint64 words in the file's Montgomery form, as read_ptau hands them over; ceremony_power defaults to power.  UNPINNED like the reader: the layout is restated
    from snarkjs's published format and no file written here has been read by snarkjs yet.  ValueError for a power outside 1..26 and an array whose shape does not
    match the power."""
    power = int(powers["power"])
    if not 1 <= power <= 26:
        raise ValueError("ptau: power outside 1..26")
    n2 = 1 << power
    secs = [(1, struct.pack("<I", 32) + BN254_Q.to_bytes(32, "little") + struct.pack("<II", power, int(powers.get("ceremony_power", power))))]
    for t, name, size in _PTAU_SECTIONS:
        points = {"tau_g1": 2 * n2 - 1, "beta_g2": 1}.get(name, n2)
        a = np.ascontiguousarray(powers[name], dtype="<u8")
        if a.size != points * size // 8:
            raise ValueError(f"ptau section {t} ({name}): {a.size * 8} bytes, the power asks for {points * size}")
        secs.append((t, a.tobytes()))
    return b"ptau" + struct.pack("<II", 1, len(secs)) + b"".join(struct.pack("<IQ", t, len(body)) + body for t, body in secs)


_G2_GENERATOR = ((10857046999023057135944570762232829481370756359578518086990519993285655852781, 11559732032986387107991004021392285783925812861821192530917403151452391805634),
                 (8495653923123431417604973247489272438418190587263600148770280649306958101930, 4082367875863433681332203403145435568316851327593401208105741076214120093531))


def new_powers(power):
    """The string nobody has contributed to (what snarkjs's `powersoftau new` starts a ceremony with): tau = alpha = beta = 1, so every point of tau_g1, alpha_g1 and
    beta_g1 is the generator of G1 and every point of tau_g2 and beta_g2 the generator of G2 — read_ptau's dictionary, rows in the file's Montgomery form.  Host,
    numpy.  Worth nothing until someone contributes (hip.contribute_powers)."""
    power = int(power)
    if not 1 <= power <= 26:
        raise ValueError("new_powers: power outside 1..26")
    row = lambda coords: np.frombuffer(b"".join((c * (1 << 256) % BN254_Q).to_bytes(32, "little") for c in coords), dtype="<u8")      # noqa: E731
    g1, g2 = row((1, 2)), row(_G2_GENERATOR[0] + _G2_GENERATOR[1])
    n2 = 1 << power
    return {"power": power, "ceremony_power": power, "tau_g1": np.tile(g1, (2 * n2 - 1, 1)), "tau_g2": np.tile(g2, (n2, 1)), "alpha_g1": np.tile(g1, (n2, 1)),
            "beta_g1": np.tile(g1, (n2, 1)), "beta_g2": np.tile(g2, (1, 1))}


_PACKED_POWERS_MAGIC = b"VPOTPK01"


def pack_powers(ctx, powers):
    """read_ptau's dictionary -> bytes of this project's own container for a string at rest, half the size of the `.ptau`'s point sections: magic "VPOTPK01", power and
    ceremony_power (u32 each), then the five arrays in _PTAU_SECTIONS order, every point packed on the GPU (hip.pack_points: x and one bit of y, canonical).  `.ptau`
    itself stays snarkjs's layout.  VimzError(ERR_INVALID): a point with a coordinate not below q or off its curve; ValueError: an array whose shape does not match
    the power."""
    from . import hip
    power = int(powers["power"])
    if not 1 <= power <= 26:
        raise ValueError("pack_powers: power outside 1..26")
    n2 = 1 << power
    parts = [_PACKED_POWERS_MAGIC + struct.pack("<II", power, int(powers.get("ceremony_power", power)))]
    for _t, name, size in _PTAU_SECTIONS:
        points = {"tau_g1": 2 * n2 - 1, "beta_g2": 1}.get(name, n2)
        a = np.ascontiguousarray(powers[name], dtype=np.uint64)
        if a.size != points * size // 8:
            raise ValueError(f"pack_powers: {name} holds {a.size * 8} bytes, the power asks for {points * size}")
        parts.append(hip.pack_points(ctx, size // 64, a, form=hip.L.FORM_MONTGOMERY).astype("<u8").tobytes())
    return b"".join(parts)


def unpack_powers(ctx, data):
    """pack_powers' bytes -> read_ptau's dictionary (rows in the file's Montgomery form; write_ptau takes it): every point unpacked on the GPU, so each is on its
    curve — subgroup membership and the string's equations remain hip.verify_powers' matter.  ValueError: not such a container or the wrong length for its power;
    VimzError(ERR_INVALID): a point that does not unpack."""
    from . import hip
    data = bytes(data)
    if len(data) < 16 or data[:8] != _PACKED_POWERS_MAGIC:
        raise ValueError("unpack_powers: not a packed powers-of-tau string")
    power, ceremony_power = struct.unpack_from("<II", data, 8)
    if not 1 <= power <= 26:
        raise ValueError("unpack_powers: power outside 1..26")
    n2 = 1 << power
    counts = [({"tau_g1": 2 * n2 - 1, "beta_g2": 1}.get(name, n2), name, size) for _t, name, size in _PTAU_SECTIONS]
    if len(data) != 16 + sum(points * size // 2 for points, _name, size in counts):
        raise ValueError(f"unpack_powers: {len(data)} bytes, the power asks for {16 + sum(points * size // 2 for points, _name, size in counts)}")
    out, pos = {"power": power, "ceremony_power": ceremony_power}, 16
    for points, name, size in counts:
        rows = np.frombuffer(data, dtype="<u8", count=points * size // 16, offset=pos).reshape(points, size // 16)
        out[name] = hip.unpack_points(ctx, size // 64, rows, form=hip.L.FORM_MONTGOMERY)
        pos += points * size // 2
    return out


def to_nova_columns(r1cs):
    """The matrices with circom wire j moved to nova-snark's column: j = 0 -> the u slot, 1 <= j <= n_pub -> X, the rest -> W.
    -> (n_witness, n_public, A, B, C)."""
    n_pub = r1cs["n_pub_out"] + r1cs["n_pub_in"]
    n_w = r1cs["n_wires"] - 1 - n_pub
    def cols(wires):
        w = wires.astype(np.int64)
        return np.where(w == 0, n_w, np.where(w <= n_pub, n_w + w, w - n_pub - 1)).astype(np.uint32)
    out = [(rows, cols(wires), vals) for rows, wires, vals in (r1cs["A"], r1cs["B"], r1cs["C"])]
    return n_w, n_pub, out[0], out[1], out[2]


def split_witness(r1cs, wtns_values):
    """One `.wtns` -> (W (n_witness, 4), X list of ints) for RelaxedAccumulator.fold."""
    n_pub = r1cs["n_pub_out"] + r1cs["n_pub_in"]
    v = np.asarray(wtns_values, dtype=np.uint64).reshape(-1, 4)
    if v.shape[0] != r1cs["n_wires"] or any(int(x) for x in v[0] ^ np.array([1, 0, 0, 0], dtype=np.uint64)):
        raise ValueError("witness does not fit the circuit (length, or wire 0 is not 1)")
    X = [sum(int(l) << (64 * i) for i, l in enumerate(row)) for row in v[1:1 + n_pub]]
    return v[1 + n_pub:], X


def _decider_key(argv):
    """decider-key FILE.ptau TRANSFORMATION RESOLUTION OUT.key [--light] [--verify] [--packed]: the decider's Groth16 key pair for that step circuit, derived from the
    string on GPU 0 (hip.Decider(powers=): tau, alpha, beta are the string's, delta is drawn here and forgotten), as vimz_decider_key_save's bytes — with --packed as
    vimz_decider_key_pack's, about half of them.  --verify: the prefixes of the string the SRS and the set-up read are judged first (hip.verify_powers); a refused
    string ends the command with VimzError."""
    light, verify, packed = "--light" in argv, "--verify" in argv, "--packed" in argv
    args = [a for a in argv if a not in ("--light", "--verify", "--packed")]
    if len(args) != 5 or any(a.startswith("--") for a in args):
        print(USAGE, file=sys.stderr)
        return 2
    from . import folding, hip
    with open(args[1], "rb") as fp:
        powers = read_ptau(fp.read())
    ctx = hip.Context(0)
    try:
        circuit, params = folding.prepare_folding(ctx, args[2], args[3], window_tables=0, backend="sonobe", powers=powers, verify_powers=verify)
        cf = hip.CycleFoldIVC(ctx, circuit, params.ck, params.secondary_key(), max_batch=1)
        try:
            dec = params.decider(cf, light=light)
            try:
                blob, info, sec = dec.save_key(packed=packed), dec.info(), dec.setup_seconds
            finally:
                dec.close()
        finally:
            cf.close(); params.free()
    finally:
        ctx.close()
    with open(args[4], "wb") as fp:
        blob.tofile(fp)
    print(f"decider-key: {'light' if light else 'full'} decider of {args[2]} {args[3]}, domain {info['domain']}, {blob.size} bytes{' (packed)' if packed else ''} -> {args[4]} (set-up {sec['total']:.1f} s)")
    return 0


def _verify(argv):
    """verify FILE.ptau [POINTS]: judges the string on GPU 0 (hip.verify_powers: POINTS of tau_g2, alpha_g1, beta_g1 and 2·POINTS − 1 of tau_g1; without POINTS the
    whole string), prints the verdict and the times; exit status 0 accepted, 1 refused."""
    if len(argv) not in (2, 3):
        print(USAGE, file=sys.stderr)
        return 2
    from . import hip
    with open(argv[1], "rb") as fp:
        powers = read_ptau(fp.read())
    n = int(argv[2]) if len(argv) == 3 else None
    sec = [0.0] * 4
    ctx = hip.Context(0)
    try:
        result, first = hip.verify_powers(ctx, powers, n, seconds=sec)
    finally:
        ctx.close()
    what = "the whole string" if n is None else f"{n} points (tau_g1: {2 * n - 1})"
    times = f"host conversion {sec[0]:.3f} s, per-point flags {sec[1]:.3f} s, combinations {sec[2]:.3f} s, pairings {sec[3]:.3f} s"
    if not result:
        print(f"verify: {argv[1]} (power {int(powers['power'])}), {what}: accepted ({times})")
        return 0
    at = f"; first: {hip.POWERS_ARRAYS[first[0]]}[{first[1]}]" if first[0] else ""
    print(f"verify: {argv[1]} (power {int(powers['power'])}), {what}: REFUSED (0x{result:x}): " + "; ".join(hip.powers_problems(result)) + f"{at} ({times})")
    return 1


def _contribute(argv):
    """contribute IN.key OUT.key RECORDS: one further delta contribution to a saved decider key on GPU 0 (hip.contribute_key: delta' is drawn here and forgotten);
    the contributed key goes to OUT.key — packed if IN.key is — and the 296-byte record is APPENDED to RECORDS (this project's own format, not snarkjs's .zkey)."""
    if len(argv) != 4:
        print(USAGE, file=sys.stderr)
        return 2
    from . import hip
    blob = np.fromfile(argv[1], dtype=np.uint8)
    sec = [0.0] * 3
    ctx = hip.Context(0)
    try:
        out, rec = hip.contribute_key(ctx, blob, seconds=sec)
    finally:
        ctx.close()
    with open(argv[2], "wb") as fp:
        out.tofile(fp)
    with open(argv[3], "ab") as fp:
        fp.write(rec.tobytes())
        n = fp.tell() // hip.KEYCHAIN_RECORD_BYTES
    print(f"contribute: {argv[1]} -> {argv[2]} ({out.size} bytes), record {n} appended to {argv[3]} (host {sec[0]:.3f} s, device {sec[1]:.3f} s)")
    return 0


def _verify_contributions(argv):
    """verify-contributions ORIGIN.key FINAL.key RECORDS: judges the chain on GPU 0 (hip.verify_key_contributions), prints the verdict and the times; exit status 0
    accepted, 1 refused.  Accepted means: FINAL.key is sound if ORIGIN.key is and any one contributor forgot their delta'.  Either key may be packed."""
    if len(argv) != 4:
        print(USAGE, file=sys.stderr)
        return 2
    from . import hip
    origin, final, records = (np.fromfile(a, dtype=np.uint8) for a in argv[1:4])
    sec = [0.0] * 4
    ctx = hip.Context(0)
    try:
        bits, first = hip.verify_key_contributions(ctx, origin, final, records, seconds=sec)
    finally:
        ctx.close()
    what = f"{argv[2]} after {records.size // hip.KEYCHAIN_RECORD_BYTES} contributions to {argv[1]}"
    times = f"host conversion {sec[0]:.3f} s, per-point flags {sec[1]:.3f} s, combination {sec[2]:.3f} s, equations {sec[3]:.3f} s"
    if not bits:
        print(f"verify-contributions: {what}: accepted ({times})")
        return 0
    at = f"; first: {hip.KEYCHAIN_PLACES[first[0]]} {first[1]}" if first[0] else ""
    print(f"verify-contributions: {what}: REFUSED (0x{bits:x}): " + "; ".join(hip.keychain_problems(bits)) + f"{at} ({times})")
    return 1


def _verify_key(argv):
    """verify-key FILE.ptau TRANSFORMATION RESOLUTION KEY [--verify]: judges on GPU 0 that KEY (vimz_decider_key_save's bytes or a packed key, from anyone) is the key a set-up from the
    string derives for that step circuit's decider — light or full as the key says —, for the delta its delta points commit to (hip.verify_key_origin); prints the
    verdict's bit names and the times; exit status 0 accepted, 1 refused.  --verify: the string's prefixes are judged first (hip.verify_powers)."""
    verify = "--verify" in argv
    args = [a for a in argv if a != "--verify"]
    if len(args) != 5 or any(a.startswith("--") for a in args):
        print(USAGE, file=sys.stderr)
        return 2
    from . import folding, hip
    with open(args[1], "rb") as fp:
        powers = read_ptau(fp.read())
    blob = np.fromfile(args[4], dtype=np.uint8)
    sec = [0.0] * 5
    ctx = hip.Context(0)
    try:
        circuit, params = folding.prepare_folding(ctx, args[2], args[3], window_tables=0, backend="sonobe", powers=powers, verify_powers=verify)
        cf = hip.CycleFoldIVC(ctx, circuit, params.ck, params.secondary_key(), max_batch=1)
        try:
            bits, first = hip.verify_key_origin(cf, powers, blob, verify_powers=verify, seconds=sec)
        finally:
            cf.close(); params.free()
    finally:
        ctx.close()
    what = f"{args[4]} against {args[1]} and the decider of {args[2]} {args[3]}"
    times = f"synthesis {sec[0]:.3f} s, host conversion {sec[1]:.3f} s, per-point flags {sec[2]:.3f} s, circuit side {sec[3]:.3f} s, combinations and pairings {sec[4]:.3f} s"
    if not bits:
        print(f"verify-key: {what}: accepted ({times})")
        return 0
    names = " ".join(n for k, n in enumerate(hip.KEYORIGIN_BIT_NAMES) if bits >> k & 1)
    at = f"; first: {hip.KEYORIGIN_PLACES[first[0]]} {first[1]}" if first[0] else ""
    print(f"verify-key: {what}: REFUSED (0x{bits:x}: {names}): " + "; ".join(hip.keyorigin_problems(bits)) + f"{at} ({times})")
    return 1


def _new_powers(argv):
    """new-powers POWER OUT.ptau: the string of tau = alpha = beta = 1 (new_powers) as a .ptau file: the origin of a ceremony.  Host only."""
    if len(argv) != 3 or not argv[1].isdigit() or not 1 <= int(argv[1]) <= 26:
        print(USAGE, file=sys.stderr)
        return 2
    data = write_ptau(new_powers(int(argv[1])))
    with open(argv[2], "wb") as fp:
        fp.write(data)
    print(f"new-powers: power {int(argv[1])}, every point a generator, {len(data)} bytes -> {argv[2]}")
    return 0


def _contribute_powers(argv):
    """contribute-powers IN.ptau OUT.ptau RECORDS: one contribution to the string on GPU 0 (hip.contribute_powers: tau', alpha', beta' are drawn here and forgotten);
    the contributed string goes to OUT.ptau and the 488-byte record is APPENDED to RECORDS (this project's own format, not snarkjs's transcript)."""
    if len(argv) != 4:
        print(USAGE, file=sys.stderr)
        return 2
    from . import hip
    with open(argv[1], "rb") as fp:
        powers = read_ptau(fp.read())
    sec = [0.0] * 3
    ctx = hip.Context(0)
    try:
        out, rec = hip.contribute_powers(ctx, powers, seconds=sec)
    finally:
        ctx.close()
    data = write_ptau(out)
    with open(argv[2], "wb") as fp:
        fp.write(data)
    with open(argv[3], "ab") as fp:
        fp.write(bytes(rec))
        n = fp.tell() // hip.POWCHAIN_RECORD_BYTES
    print(f"contribute-powers: {argv[1]} -> {argv[2]} (power {int(powers['power'])}, {len(data)} bytes), record {n} appended to {argv[3]} (host {sec[0]:.3f} s, device {sec[1]:.3f} s)")
    return 0


def _verify_powers_contributions(argv):
    """verify-powers-contributions ORIGIN.ptau FINAL.ptau RECORDS: judges the chain on GPU 0 (hip.verify_powers_contributions), prints the verdict's bit names and the
    times; exit status 0 accepted, 1 refused.  Accepted means: FINAL.ptau is the powers of one tau with consistent alpha and beta, unknown to everyone if any one
    contributor forgot their secrets."""
    if len(argv) != 4:
        print(USAGE, file=sys.stderr)
        return 2
    from . import hip
    with open(argv[1], "rb") as fp:
        origin = read_ptau(fp.read())
    with open(argv[2], "rb") as fp:
        final = read_ptau(fp.read())
    records = np.fromfile(argv[3], dtype=np.uint8)
    sec = [0.0] * 3
    ctx = hip.Context(0)
    try:
        bits, sbits, first = hip.verify_powers_contributions(ctx, origin, final, records, seconds=sec)
    finally:
        ctx.close()
    what = f"{argv[2]} after {records.size // hip.POWCHAIN_RECORD_BYTES} contributions to {argv[1]}"
    times = f"points {sec[0]:.3f} s, knowledge {sec[1]:.3f} s, the string {sec[2]:.3f} s"
    if not bits:
        print(f"verify-powers-contributions: {what}: accepted ({times})")
        return 0
    names = " ".join(hip.POWCHAIN_BIT_NAMES[k] for k in range(len(hip.POWCHAIN_BIT_NAMES)) if bits >> k & 1)
    inner = f"; the string: 0x{sbits:x}: " + "; ".join(hip.powers_problems(sbits)) if sbits else ""
    at = f"; first: {hip.POWCHAIN_PLACES[first[0]]} {first[1]}" if first[0] else ""
    print(f"verify-powers-contributions: {what}: REFUSED (0x{bits:x}: {names}): " + "; ".join(hip.powchain_problems(bits)) + f"{inner}{at} ({times})")
    return 1


def _pack_key(argv):
    """pack-key IN OUT / unpack-key IN OUT: a saved decider key to its packed form (hip.pack_key: every point as x and one bit of y, about half the bytes) and back
    (hip.unpack_key: vimz_decider_key_save's bytes, byte for byte) on GPU 0.  A point that is refused ends the command with VimzError."""
    if len(argv) != 3:
        print(USAGE, file=sys.stderr)
        return 2
    from . import hip
    blob = np.fromfile(argv[1], dtype=np.uint8)
    ctx = hip.Context(0)
    try:
        out = (hip.pack_key if argv[0] == "pack-key" else hip.unpack_key)(ctx, blob)
    finally:
        ctx.close()
    with open(argv[2], "wb") as fp:
        out.tofile(fp)
    print(f"{argv[0]}: {argv[1]} ({blob.size} bytes) -> {argv[2]} ({out.size} bytes)")
    return 0


def _pack_powers(argv):
    """pack-powers FILE.ptau OUT: the string in this project's packed container (pack_powers) on GPU 0.  unpack-powers IN FILE.ptau: back to a `.ptau` (unpack_powers,
    write_ptau).  A point that is refused ends the command with VimzError."""
    if len(argv) != 3:
        print(USAGE, file=sys.stderr)
        return 2
    from . import hip
    with open(argv[1], "rb") as fp:
        data = fp.read()
    ctx = hip.Context(0)
    try:
        out = pack_powers(ctx, read_ptau(data)) if argv[0] == "pack-powers" else write_ptau(unpack_powers(ctx, data))
    finally:
        ctx.close()
    with open(argv[2], "wb") as fp:
        fp.write(out)
    print(f"{argv[0]}: {argv[1]} ({len(data)} bytes) -> {argv[2]} ({len(out)} bytes)")
    return 0


USAGE = ("usage: python -m vimz_amd.iden3 lagrange FILE.ptau LOGN OUT.npz\n"
         "       python -m vimz_amd.iden3 new-powers POWER OUT.ptau\n"
         "       python -m vimz_amd.iden3 contribute-powers IN.ptau OUT.ptau RECORDS\n"
         "       python -m vimz_amd.iden3 verify-powers-contributions ORIGIN.ptau FINAL.ptau RECORDS\n"
         "       python -m vimz_amd.iden3 decider-key FILE.ptau TRANSFORMATION RESOLUTION OUT.key [--light] [--verify] [--packed]\n"
         "       python -m vimz_amd.iden3 verify FILE.ptau [POINTS]\n"
         "       python -m vimz_amd.iden3 contribute IN.key OUT.key RECORDS\n"
         "       python -m vimz_amd.iden3 verify-contributions ORIGIN.key FINAL.key RECORDS\n"
         "       python -m vimz_amd.iden3 verify-key FILE.ptau TRANSFORMATION RESOLUTION KEY [--verify]\n"
         "       python -m vimz_amd.iden3 pack-key IN.key OUT\n"
         "       python -m vimz_amd.iden3 unpack-key IN OUT.key\n"
         "       python -m vimz_amd.iden3 pack-powers FILE.ptau OUT\n"
         "       python -m vimz_amd.iden3 unpack-powers IN FILE.ptau\n"
         "(the key commands take a key in either form, vimz_decider_key_save's or packed)")


def _main(argv):
    """python -m vimz_amd.iden3 lagrange FILE.ptau LOGN OUT.npz: the string's Lagrange bases over the domain of 2^LOGN points (hip.lagrange_from_powers, on GPU 0)
    as an .npz of tau_g1, alpha_g1, beta_g1 (n, 8) and tau_g2 (n, 16) in the file's Montgomery form, with logn.
    python -m vimz_amd.iden3 decider-key ...: _decider_key.  python -m vimz_amd.iden3 verify ...: _verify.
    python -m vimz_amd.iden3 contribute ... / verify-contributions ... / verify-key ...: _contribute, _verify_contributions, _verify_key.
    python -m vimz_amd.iden3 new-powers ... / contribute-powers ... / verify-powers-contributions ...: _new_powers, _contribute_powers, _verify_powers_contributions.
    python -m vimz_amd.iden3 pack-key ... / unpack-key ...: _pack_key.  python -m vimz_amd.iden3 pack-powers ... / unpack-powers ...: _pack_powers."""
    if argv and argv[0] in ("pack-key", "unpack-key"):
        return _pack_key(argv)
    if argv and argv[0] in ("pack-powers", "unpack-powers"):
        return _pack_powers(argv)
    if argv and argv[0] == "new-powers":
        return _new_powers(argv)
    if argv and argv[0] == "contribute-powers":
        return _contribute_powers(argv)
    if argv and argv[0] == "verify-powers-contributions":
        return _verify_powers_contributions(argv)
    if argv and argv[0] == "verify-key":
        return _verify_key(argv)
    if argv and argv[0] == "decider-key":
        return _decider_key(argv)
    if argv and argv[0] == "verify":
        return _verify(argv)
    if argv and argv[0] == "contribute":
        return _contribute(argv)
    if argv and argv[0] == "verify-contributions":
        return _verify_contributions(argv)
    if len(argv) != 4 or argv[0] != "lagrange":
        print(USAGE, file=sys.stderr)
        return 2
    from . import hip
    with open(argv[1], "rb") as fp:
        powers = read_ptau(fp.read())
    logn = int(argv[2])
    ctx = hip.Context(0)
    try:
        bases = hip.lagrange_from_powers(ctx, powers, logn)
    finally:
        ctx.close()
    with open(argv[3], "wb") as fp:          # (a file object: savez leaves its name alone)
        np.savez(fp, logn=np.int64(logn), **bases)
    print(f"lagrange: {1 << logn} points each of tau_g1, alpha_g1, beta_g1, tau_g2 -> {argv[3]}")
    return 0


if __name__ == "__main__":
    sys.exit(_main(sys.argv[1:]))
