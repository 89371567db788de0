"""Record tests/golden/slanet_decode.json from the reference's own TableLabelDecode (model/slanet/table_postprocess.py, loaded by file path: the module
needs only numpy and torch).

    python tests/golden/make_slanet_golden.py /path/to/reference/src/pdftable/model/slanet/table_postprocess.py

Per language (en: V = 30, L = 4; ch: V = 50, L = 8; the hand-written dictionaries of tests/golden/slanet/) five tables of T = 10 steps:
  0  eos at step 0 (not a stop: the reference's rule is idx > 0), tokens after it, eos again at step 6
  1  eos at step 1 behind one cell token
  2  eos never: all T steps are tokens
  3  an sos in the middle of the sequence (skipped, its box too)
  4  the empty table: sos at step 0, eos at step 1
Inputs are stored as the float32 tensors the decode reads (structure_probs [B, T, V], loc_preds [B, T, L], shape_list [B, 6]); outputs as it returns them."""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
T = 10


def load_reference(path):
    spec = importlib.util.spec_from_file_location("slanet_table_postprocess", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sequences(dec, rng):
    """five id sequences [5, T] over the decode's own table (`dec.character`)"""
    V = len(dec.character)
    sos, eos = dec.dict["sos"], dec.dict["eos"]
    cell = [dec.dict[t] for t in ("<td", "<td></td>") if t in dec.dict]
    plain = [i for i in range(1, V - 1)]
    ids = rng.choice(plain, size=(5, T))
    ids[:, 2] = cell[0]
    ids[:, 4] = cell[-1]
    ids[0, 0], ids[0, 6] = eos, eos
    ids[1, 0], ids[1, 1] = cell[-1], eos
    ids[3, 3] = sos
    ids[4, 0], ids[4, 1] = sos, eos
    return ids


def main(ref_path):
    ref = load_reference(ref_path)
    out = {}
    for lang, L in (("en", 4), ("ch", 8)):
        dict_path = os.path.join(HERE, "slanet", "table_structure_dict%s.txt" % ("_ch" if lang == "ch" else ""))
        dec = ref.TableLabelDecode(character_dict_path=dict_path, merge_no_span_structure=True)
        V = len(dec.character)
        rng = np.random.default_rng(7 if lang == "en" else 8)
        ids = sequences(dec, rng)
        logits = rng.normal(0.0, 1.0, (5, T, V))
        np.put_along_axis(logits, ids[..., None], 6.0 + rng.uniform(0.0, 2.0, (5, T, 1)), axis=2)
        e = np.exp(logits - logits.max(-1, keepdims=True))
        probs = (e / e.sum(-1, keepdims=True)).astype(np.float32)
        assert np.array_equal(probs.argmax(2), ids)
        loc = rng.uniform(0.0, 1.0, (5, T, L)).astype(np.float32)
        shape_list = np.array([[3, 5, 97.6, 97.6, 488, 488], [200, 200, 2.44, 2.44, 488, 488], [976, 640, 0.5, 0.5, 488, 488], [100, 333, 1.4654654, 1.4654654, 488, 488],
                               [50, 60, 8.1333333, 8.1333333, 488, 488]], dtype=np.float32)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")             # np.mean([]) of the empty table
            res = dec({"structure_probs": probs.copy(), "loc_preds": loc.copy()}, [shape_list])
        out[lang] = {
            "V": V, "L": L, "characters": dec.character,
            "structure_probs": probs.tolist(), "loc_preds": loc.tolist(), "shape_list": shape_list.tolist(),
            "structure_batch_list": [[toks, None if np.isnan(score) else float(score)] for toks, score in res["structure_batch_list"]],
            "bbox_batch_list": [np.asarray(b, np.float32).reshape(-1, L).tolist() for b in res["bbox_batch_list"]],
        }
    with open(os.path.join(HERE, "slanet_decode.json"), "w") as f:
        json.dump(out, f)
    print({k: (v["V"], [len(s[0]) for s in v["structure_batch_list"]]) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
