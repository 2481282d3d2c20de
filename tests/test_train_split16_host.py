"""Option "train_split16" (include/dcscn.h), host side (no GPU): the --train_split16 switch and the eligibility rule's cases."""
import train_split16_cases as C
from test_host import _flags


def test_train_split16_flag_parses_and_defaults_to_false(tmp_path):
    from helper import args
    from dcscn_amd.model import SuperResolution
    assert "train_split16" in args.FLAGS
    flag = args.FLAGS._flags["train_split16"]
    assert flag.default is False and flag.kind == "boolean" and args.FLAGS.train_split16 is False
    saved = (flag.value, flag.present, args.FLAGS.is_parsed())
    try:
        assert args.FLAGS(["prog", "--train_split16"]) == ["prog"] and args.FLAGS.train_split16 is True
        assert args.FLAGS(["prog", "--notrain_split16"]) == ["prog"] and args.FLAGS.train_split16 is False
    finally:
        flag.value, flag.present = saved[0], saved[1]
        object.__setattr__(args.FLAGS, "_parsed", saved[2])
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models")))
    assert m.train_split16 is False
    m = SuperResolution(_flags(checkpoint_dir=str(tmp_path / "models"), train_split16=True))
    assert m.train_split16 is True


def test_the_cases_cover_eligible_mixed_and_narrow_nets(oracle):
    layers = lambda over: [(op["var"], op["cin"], op["cout"]) for op in oracle.build_topology(oracle.make_config(**over)) if op["op"] == "conv"]
    for over in (C.ODD, C.K5, C.X4R, C.MIXED):
        on = [v for v, ci, co in layers(over) if C.eligible(ci, co)]
        off = [v for v, ci, co in layers(over) if not C.eligible(ci, co)]
        assert on and off, over                                     # (CNN1 and the last conv are never eligible)
    assert any(ci % 8 and co % 8 for _, ci, co in layers(C.ODD) if C.eligible(ci, co))
    ups = [(ci, co) for v, ci, co in layers(C.X4R) if v.startswith("Up-PS")]
    assert len(ups) == 2 and all(C.eligible(ci, co) for ci, co in ups)
    hr = [(ci, co) for v, ci, co in layers(C.X4R) if v.startswith("R-CNN")]
    assert sum(C.eligible(ci, co) for ci, co in hr) == 2
    assert not [v for v, ci, co in layers(C.NARROW) if C.eligible(ci, co)]
    assert {c[1] for c in C.CASES.values()} == {"prelu", "relu", "selu"}
    assert {c[3] for c in C.CASES.values()} == {1.0, 0.8} and {c[4] for c in C.CASES.values()} == {False, True}
