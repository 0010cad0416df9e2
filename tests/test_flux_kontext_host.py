"""CPU tests of the FLUX.1 Kontext host layer (`mi355_flow.flux`: `FluxKontextRolloutMixin`, `split_kontext_ids`, the standalone adapter;
`mi355_flow.samples.Flux1KontextSample`) against the reference's `Flux1KontextAdapter` (models/flux/flux1_kontext.py): the parameter lists
of `inference()` / `forward()` are the ABI (the trainer filters its kwargs by signature), the ids the engine would not reproduce are
refused, the sample class carries the reference's fields."""
import ast
import dataclasses
import inspect
import os

import pytest
import torch

SHAPES = [(8, 8, 8, 8), (6, 10, 10, 4), (16, 16, 8, 12)]       # target latent h, w / condition latent h, w


_NO_DEFAULT = "<no default>"


def _reference_signature(fn_name):
    """[(name, default)] of `Flux1KontextAdapter.<fn_name>`, read from the source with `ast` (nothing is imported)."""
    from oracle import ref_package
    path = os.path.join(ref_package.REF_SRC, "flow_factory", "models", "flux", "flux1_kontext.py")
    if not os.path.isfile(path):
        pytest.skip("needs the reference tree (build container only)")
    tree = ast.parse(open(path).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Flux1KontextAdapter")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == fn_name)
    a = fn.args
    assert not a.posonlyargs and not a.kwonlyargs and a.vararg is None and a.kwarg is None
    defaults = [_NO_DEFAULT] * (len(a.args) - len(a.defaults)) + [ast.literal_eval(d) for d in a.defaults]
    return list(zip([arg.arg for arg in a.args], defaults))


@pytest.mark.parametrize("fn_name", ["inference", "forward"])
def test_mixin_signatures_equal_the_reference(fn_name):
    """Parameter names, order and defaults: the trainer filters its kwargs by `inspect.signature`, so the parameter list is the ABI."""
    from mi355_flow.flux import FluxKontextRolloutMixin
    want = _reference_signature(fn_name)
    sig = inspect.signature(getattr(FluxKontextRolloutMixin, fn_name))
    got = [(n, _NO_DEFAULT if p.default is inspect.Parameter.empty else p.default) for n, p in sig.parameters.items()]
    assert got == want
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())


def _ids(hp, wp, lead=0.0):
    from mi355_flow.flux import prepare_latent_image_ids
    ids = prepare_latent_image_ids(hp, wp, "cpu", torch.float32)
    ids[:, 0] = lead
    return ids


@pytest.mark.parametrize("h,w,ch,cw", SHAPES)
def test_split_kontext_ids_round_trips(h, w, ch, cw):
    from mi355_flow.flux import split_kontext_ids
    ids = torch.cat([_ids(h // 2, w // 2), _ids(ch // 2, cw // 2, 1.0)])
    assert split_kontext_ids(ids) == (h // 2, w // 2, ch // 2, cw // 2)
    assert split_kontext_ids(ids.bfloat16()) == (h // 2, w // 2, ch // 2, cw // 2)      # the dtype the rollout stores them in


def test_split_kontext_ids_refuses_what_the_engine_would_not_reproduce():
    from mi355_flow.flux import split_kontext_ids
    tgt, cond = _ids(4, 4), _ids(4, 6, 1.0)
    good = torch.cat([tgt, cond])
    split_kontext_ids(good)
    shuffled = torch.cat([tgt, cond[torch.randperm(len(cond), generator=torch.Generator().manual_seed(1))]])
    with pytest.raises(ValueError, match="condition rows"):
        split_kontext_ids(shuffled)
    with pytest.raises(ValueError, match="condition rows"):
        split_kontext_ids(torch.cat([tgt, cond, cond]))                  # two condition images under the same first id
    with pytest.raises(ValueError, match=r"first ids \[0.0, 1.0, 2.0\]"):
        split_kontext_ids(torch.cat([tgt, cond, _ids(4, 6, 2.0)]))       # ... or under a first id of 2
    offset = cond.clone()
    offset[:, 2] += 4                                                     # the condition grid placed beside the target's
    with pytest.raises(ValueError, match="cols 4..9"):
        split_kontext_ids(torch.cat([tgt, offset]))
    with pytest.raises(ValueError, match="target rows must come first"):
        split_kontext_ids(torch.cat([cond, tgt]))
    with pytest.raises(ValueError, match=r"first ids \[0.0\]"):
        split_kontext_ids(tgt)                                            # no condition at all
    with pytest.raises(ValueError, match="target rows"):
        split_kontext_ids(torch.cat([tgt[:-1], cond]))                    # a target row missing


def test_flux1_kontext_sample_fields():
    from mi355_flow.samples import BaseSample, Flux1KontextSample
    names = {f.name for f in dataclasses.fields(Flux1KontextSample)}
    assert {"pooled_prompt_embeds", "image_latents", "latent_ids", "condition_images"} <= names
    assert vars(Flux1KontextSample)["_shared_fields"] == frozenset({"latent_ids"})
    assert Flux1KontextSample.shared_fields() == BaseSample._shared_fields | {"latent_ids"}
    assert "condition_images" in Flux1KontextSample._id_fields
    ids = torch.cat([_ids(2, 2), _ids(2, 3, 1.0)])
    mk = lambda v: Flux1KontextSample(prompt="p", image_latents=torch.full((6, 64), v), latent_ids=ids, condition_images=torch.full((3, 8, 8), v),
                                      all_latents=torch.zeros(2, 4, 64))
    a, b = mk(0.25), mk(0.75)
    assert isinstance(a.condition_images, list) and a.condition_images[0].shape == (3, 8, 8)
    assert a.unique_id != b.unique_id and a.unique_id == mk(0.25).unique_id        # the condition image is part of the group identity
    st = Flux1KontextSample.stack([a, b])
    assert st["latent_ids"] is ids and st["image_latents"].shape == (2, 6, 64) and st["all_latents"].shape == (2, 2, 4, 64)


def test_standalone_adapter_needs_the_encoded_condition():
    """No native VAE encoder: `images=` without `image_latents` / `image_ids` raises with that message (checked on the method: constructing
    the adapter needs a GPU)."""
    from mi355_flow.flux import Flux1KontextNativeAdapter, FluxKontextRolloutMixin, FluxRolloutMixin
    assert issubclass(Flux1KontextNativeAdapter, FluxKontextRolloutMixin) and issubclass(FluxKontextRolloutMixin, FluxRolloutMixin)
    assert Flux1KontextNativeAdapter.inference is FluxKontextRolloutMixin.inference
    ad = object.__new__(Flux1KontextNativeAdapter)
    with pytest.raises(RuntimeError, match="no VAE encoder.*image_latents, image_ids, not images="):
        ad.encode_image(images=[torch.zeros(3, 16, 16)])

    class _Sched:
        dynamics_type = "ODE"

    ad.device, ad._live_weights, ad.scheduler = torch.device("cpu"), None, _Sched()
    pe, pp = torch.zeros(1, 4, 8), torch.zeros(1, 8)
    with pytest.raises(RuntimeError, match="no VAE encoder"):
        ad.inference(images=[torch.zeros(3, 16, 16)], prompt_embeds=pe, pooled_prompt_embeds=pp)
    with pytest.raises(RuntimeError, match="no VAE encoder"):             # half an encoded condition is none
        ad.inference(images=[torch.zeros(3, 16, 16)], prompt_embeds=pe, pooled_prompt_embeds=pp, image_latents=torch.zeros(1, 4, 64))


def test_plugin_exports_the_kontext_adapter():
    """The Flow-Factory binding names the class; without an importable `flow_factory` it is the `_unavailable` placeholder."""
    import mi355_flow.flow_factory_plugin as plugin
    assert hasattr(plugin, "Flux1KontextNativeAdapter")
    if plugin._RefAdapter is None:
        with pytest.raises(ImportError, match="mi355_flow.flux.Flux1KontextNativeAdapter"):
            plugin.Flux1KontextNativeAdapter(None, None)
