"""The model folder's parameters.json "type" -> the model class that loads it (the mapping the reference's apply_cae,
train_cae --continue-training and ModelEvaluator each spell out: model_evaluator.py:64-72)."""
import json
import os


def model_classes():
    from .conv_ae_model import ConvAEModel
    from .linear_model import LinearModel
    from .unet import UNET
    from .var_ae_model import VarAEModel
    return {"ConvAEModel": ConvAEModel, "UNET": UNET, "VarAEModel": VarAEModel, "LinearModel": LinearModel}


def read_parameters(model_folder):
    with open(os.path.join(model_folder, "parameters.json")) as f:
        return json.loads(f.read())


def load_model(model_folder):
    """a model of the folder's type with its weights, normalisation and history loaded"""
    kinds = model_classes()
    kind = read_parameters(model_folder)["type"]
    if kind not in kinds:
        raise SystemExit(f"cae_tools_amd implements {sorted(kinds)}; model folder holds a {kind}")
    model = kinds[kind]()
    model.load(model_folder)
    return model
