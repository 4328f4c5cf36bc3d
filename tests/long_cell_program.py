"""A two-class program with a free-text column: one cell longer than 255 characters switches its column's pair table to
16-bit distances (pclean_build_pair_table: elem_bytes == 2), and every scorer that reads the table then takes its other
load branch.  For tests/test_gpu_long_cells.py (sweeps on the device against the CPU oracle) and
tests/test_long_cells_cpu.py (the power of that comparison, on the oracle alone).

  Ent:  name ~ StringPrior(3, 12, observed names)     5 - 9 letters
        note ~ ChooseUniformly(observed notes)        20 - 60 characters; the notes of entities LONG_ENTS have 256, 277
                                                      and 300
  Obs:  ent -> Ent;  name ~ AddTypos(ent.name);  note ~ AddTypos(ent.note)

(note is no StringPrior: the lowering refuses a StringPrior whose max_length exceeds 255 by name, refused_program below,
and under StringPrior(.., 255, ..) a latent note of 256 characters and more has probability zero.)

N_ENT entities, ROWS_PER rows each.  The first row of an entity is clean (so that every clean value is a possible latent
value); the others carry typos, in the long cells too (up to six edits there), some cells are missing, and row STRANGER's
note is an unrelated string of 280 characters (more than 255 edits from everything short).  `tile` repeats the rows (the
same cells again: the tables do not grow) for launches of more than 1 024 items; `n_latent` fills the latent table with
that many rows, entity e holding the values of entity e % N_ENT, for candidate lists beyond what the LDS-resident
enumeration keeps.

The flat twins (own blocks of the observed class, tests/own_choice_program.py's and tests/own_product_program.py's
conventions, so that their exact_scores / exact_matrix serve as the reference):

  flat_long()          note ~ ChooseProportionally(notes, p);  note_obs ~ AddTypos(note)
  flat_long_product()  a ~ ChooseProportionally(notes, pa);  b ~ ChooseProportionally(names, theta, index="a");
                       a_obs ~ AddTypos(a);  b_obs ~ AddTypos(b)      — the product leaf's index column is the long one

over the notes / names of FLAT_ENTS (the three long entities and seven short ones) and their rows of the base table."""
import numpy as np

from pclean_amd.model import AddTypos, ChooseUniformly, LoweredModel, Model, Query, StringPrior
from pclean_amd.trace import Trace

LETTERS = np.array(list("abcdefghijklmnopqrstuvwxyz "))
N_ENT, ROWS_PER = 40, 3
LONG_ENTS = {3: 256, 17: 277, 31: 300}
STRANGER = 17 * ROWS_PER + 2       # a row of a long entity ...
SHORT_STRANGER = 8 * ROWS_PER + 1  # ... and one of a short entity get an unrelated long note
FLAT_ENTS = (3, 17, 31, 0, 8, 12, 20, 25, 33, 39)


def _rand(rng, lo, hi):
    s = "".join(rng.choice(LETTERS, int(rng.integers(lo, hi + 1)))).strip()
    return s if len(s) >= lo else s + "x" * (lo - len(s))


def _typos(rng, s, k):
    c = list(s)
    for _ in range(k):
        kind = int(rng.integers(0, 4))
        if kind == 0:
            c.insert(int(rng.integers(0, len(c) + 1)), str(rng.choice(LETTERS[:26])))
        elif kind == 1 and len(c) > 1:
            del c[int(rng.integers(0, len(c)))]
        elif kind == 2 and len(c) > 1:
            q = int(rng.integers(0, len(c) - 1))
            c[q], c[q + 1] = c[q + 1], c[q]
        elif c:
            c[int(rng.integers(0, len(c)))] = str(rng.choice(LETTERS[:26]))
    return "".join(c)


def long_cell_data(seed=7):
    """(entities, dirty columns, owner of every row) of the base table"""
    rng = np.random.default_rng(seed)
    ents = []
    for e in range(N_ENT):
        n = LONG_ENTS.get(e)
        ents.append({"name": _rand(rng, 5, 9), "note": _rand(rng, n, n) if n else _rand(rng, 20, 60)})
    dirty, owner = {"NAME": [], "NOTE": []}, []
    for e, ent in enumerate(ents):
        for r in range(ROWS_PER):
            i = e * ROWS_PER + r
            name, note = ent["name"], ent["note"]
            if r > 0:
                name = _typos(rng, name, int(rng.integers(0, 3)))
                note = _typos(rng, note, int(rng.integers(1, 7)) if e in LONG_ENTS else int(rng.integers(0, 4)))
                if i % 11 == 4:
                    name = None
                if i % 13 == 7:
                    note = None
            if i in (STRANGER, SHORT_STRANGER):
                note = _rand(rng, 280, 280)
            dirty["NAME"].append(name)
            dirty["NOTE"].append(note)
            owner.append(e)
    return ents, dirty, owner


def _model(dirty, note_prior, name_prior=None):
    m = Model()
    c = m.add_class("Ent")
    names = list(dict.fromkeys(v for v in dirty["NAME"] if v is not None))
    c.choice("name", name_prior(names) if name_prior else StringPrior(3, 12, names))
    c.choice("note", note_prior(list(dict.fromkeys(v for v in dirty["NOTE"] if v is not None))))
    o = m.add_class("Obs")
    with o.block():
        o.fk("ent", "Ent")
        o.choice("name", AddTypos("ent.name"))
        o.choice("note", AddTypos("ent.note"))
    return m, c, Query(m, "Obs", {"NAME": ("ent.name", "name"), "NOTE": ("ent.note", "note")})


def refused_program(seed=7):
    """the same program with note ~ StringPrior(10, 300, observed notes): (model, query, dirty) for LoweredModel, which
    refuses it"""
    _, dirty, _ = long_cell_data(seed)
    m, _, q = _model(dirty, lambda atoms: StringPrior(10, 300, atoms))
    return m, q, dirty


def long_cell_setup(seed=7, tile=1, n_latent=None, uniform_names=False):
    """uniform_names: name ~ ChooseUniformly(observed names) — no created row can hold a ProposalDummyValue, which the
    device-resident commit refuses"""
    ents, dirty, owner = long_cell_data(seed)
    dirty = {c: v * tile for c, v in dirty.items()}
    owner = owner * tile
    m, c, q = _model(dirty, ChooseUniformly, ChooseUniformly if uniform_names else None)
    if n_latent is not None:
        c.py_strength = n_latent / 16.0  # (among thousands of rows no draw would take the new-row candidate otherwise)
    lw = LoweredModel(m, q, dirty)
    obs = lw.encode_observations(dirty)
    n = obs.shape[1]
    if n_latent is None:
        tr = Trace.from_clean_values(lw, {0: {f: [ents[k][f] for k in owner] for f in ("name", "note")}}, n, seed)
    else:
        tr = Trace(lw, n, seed)
        vals = np.zeros((n_latent, len(lw.layout["Ent"])), dtype=np.int32)
        for f in ("name", "note"):
            dom = lw.latent_dom[("Ent", f)]
            col = np.array([dom.get(e[f]) for e in ents], dtype=np.int32)
            assert (col >= 0).all()
            vals[:, lw.colidx["Ent"][f]] = col[np.arange(n_latent) % N_ENT]
        ids = tr.insert_rows_bulk("Ent", vals)
        tr.cur[0] = ids[np.array(owner)]
        t = tr.tables["Ent"]
        t.counts[:t.n] += np.bincount(tr.cur[0], minlength=t.n)
    return dict(ents=ents, dirty=dirty, owner=owner, lw=lw, obs=obs, trace=tr)


def pair_ids(lw):
    """(pair table id, observed domain, latent domain) of the name and of the note term"""
    out = {}
    lw.pool.arrays()  # (the pool's lengths are built with its arrays)
    for key, (pid, odom, ldom) in lw.pair_id.items():
        longest = max(int(lw.pool.lens[odom.id_array()].max()), int(lw.pool.lens[ldom.id_array()].max()))
        out["note" if longest > 255 else "name"] = (pid, odom, ldom)
    assert set(out) == {"name", "note"}
    return out


def bytes_of_a_16bit_table(table):
    """what a scorer that takes the 8-bit load on a 16-bit table reads: entry [u][v] = byte u * n_lat + v of the buffer
    (little endian: the low bytes of the first half of the entries, interleaved with their high bytes)"""
    t = np.ascontiguousarray(table, dtype="<u2")
    return t.view(np.uint8).ravel()[:t.size].reshape(t.shape).astype(np.uint16)


def _flat_rows(seed):
    ents, dirty, owner = long_cell_data(seed)
    rows = [i for i, e in enumerate(owner) if e in FLAT_ENTS]
    return [ents[e] for e in FLAT_ENTS], {c: [v[i] for i in rows] for c, v in dirty.items()}


def flat_long(seed=7):
    """own_choice_program's spec of the flat twin (exact_scores, exact_rows and lower take it)"""
    import own_choice_program as ocp
    from pclean_amd.model import ChooseProportionally, ProportionsParameter
    ents, dirty = _flat_rows(seed)
    notes = [e["note"] for e in ents]
    m = Model()
    o = m.add_class("Obs")
    o.param("p", ProportionsParameter(1.0))
    with o.block():
        o.choice("note", ChooseProportionally(notes, "p"))
        o.choice("note_obs", AddTypos("note"))
    q = Query(m, "Obs", {"Note": ("note", "note_obs")})
    return ocp._spec(m, q, {"Note": dirty["NOTE"]}, {"note": notes}, {"note": [("Note", "typos", None)]})


def flat_long_product(seed=7):
    """own_product_program's spec (flatp's keys) with A = the notes, B = the names"""
    import own_product_program as opp
    ents, dirty = _flat_rows(seed)
    A, B = [e["note"] for e in ents], [e["name"] for e in ents]
    d = {"Degree": dirty["NOTE"], "Spec": dirty["NAME"]}
    m, q = opp.model(A, B)
    return dict(model=m, query=q, dirty=d, A=A, B=B, n_rows=len(d["Degree"]), variant=False, direct={},
                terms={"a": [("Degree", "typos", None)], "b": [("Spec", "typos", None)]})


def flat_long_twin(S):
    """the same choice behind a slot (own_choice_program.twin1's shape): its new-row leaf (block 0, node 1) is the path
    these rows took before own blocks existed"""
    from pclean_amd.model import ChooseProportionally, ProportionsParameter
    m = Model()
    a = m.add_class("A")
    a.param("p", ProportionsParameter(1.0))
    a.choice("x", ChooseProportionally(S["choices"]["note"], "p"))
    o = m.add_class("Obs")
    o.fk("r", "A")
    o.choice("note_obs", AddTypos("r.x"))
    return dict(model=m, query=Query(m, "Obs", {"Note": ("r.x", "note_obs")}), dirty=S["dirty"], n_rows=S["n_rows"], leaf=(0, 1))
