"""Every YAML recipe the reference ships under options/{train,test}/** goes through the product's option loader and
constructs the product's objects: EDLoRATrainer(**opt['models']) with a synthetic `pretrained_path` (no
checkpoints exist offline), the three AdamW groups of TrainEngine from opt['train'], the `instance_transform` chain of the
dataset block, the PromptDataset of the validation block. The recipes and the validation prompt files they name are stored
unmodified under tests/golden/reference_recipes/, in the reference's directory layout."""
import glob
import os

import pytest
import torch

REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_recipes')
TRAIN = sorted(glob.glob(os.path.join(REF, 'options', 'train', '**', '*.yml'), recursive=True))
TEST = sorted(glob.glob(os.path.join(REF, 'options', 'test', '**', '*.yml'), recursive=True))
assert len(TRAIN) == 6 and len(TEST) == 3, (TRAIN, TEST)     # every recipe the reference ships

# the option surface the product reads (and the reference's recipes use); anything else in a shipped recipe is a gap
TOP_KEYS = {'name', 'manual_seed', 'mixed_precision', 'gradient_accumulation_steps', 'datasets', 'models', 'path', 'train', 'val',
            'logger'}
MODEL_KEYS = {'pretrained_path', 'enable_edlora', 'finetune_cfg', 'new_concept_token', 'initializer_token', 'noise_offset',
              'attn_reg_weight', 'reg_full_identity', 'use_mask_loss', 'gradient_checkpoint', 'enable_xformers'}


@pytest.mark.parametrize('path', TRAIN, ids=[os.path.basename(p)[:28] for p in TRAIN])
def test_reference_train_recipe_builds_the_product_objects(emulated_hip, path):
    from mixofshow.data.pil_transform import PairCompose, build_transform
    from mixofshow.data.prompt_dataset import PromptDataset
    from mixofshow.pipelines.train_loop import TrainEngine
    from mixofshow.pipelines.trainer_edlora import EDLoRATrainer
    from mixofshow.utils.options import load_options
    opt = load_options(path)
    assert set(opt) <= TOP_KEYS, f'unknown top-level keys {set(opt) - TOP_KEYS}'
    assert set(opt['models']) <= MODEL_KEYS, f'unknown model keys {set(opt["models"]) - MODEL_KEYS}'
    models = dict(opt['models'], pretrained_path='synthetic://tiny')
    torch.manual_seed(opt['manual_seed'])
    tr = EDLoRATrainer(**models)
    fc = opt['models']['finetune_cfg']
    n_words = len(opt['models']['new_concept_token'].split('+'))
    assert tr.concept_embedding.shape[0] == 16 * n_words and tr.enable_edlora == opt['models']['enable_edlora']
    assert len(tr.unet_lora) > 0 and len(tr.text_encoder_lora) > 0
    assert all(l.lora_down.weight.shape[0] == fc['unet']['lora_cfg']['rank'] for l in tr.unet_lora)
    assert tr.attn_reg_weight == opt['models']['attn_reg_weight'] and tr.use_mask_loss == opt['models']['use_mask_loss']
    train_cfg = opt['datasets']['train']
    total_iter = 10 * train_cfg['dataset_enlarge_ratio'] / (train_cfg['batch_size_per_gpu'] * 2)
    engine = TrainEngine(tr, opt['train'], total_iter, 'no', opt.get('gradient_accumulation_steps', 1))
    lrs = [g['lr'] for g in engine.optimizer.param_groups]
    assert lrs == [fc['text_embedding']['lr'], fc['text_encoder']['lr'], fc['unet']['lr']]          # three groups, recipe order
    assert engine.threshold == opt['train']['emb_norm_threshold']
    assert engine.optimizer.param_groups[0]['weight_decay'] == opt['train']['optim_g']['weight_decay']
    chain = PairCompose([build_transform(t) for t in train_cfg['instance_transform']])
    assert [type(t).__name__ for t in chain.transforms] == [t['type'] for t in train_cfg['instance_transform']]
    # the validation block: prompts come from the reference's own prompt files
    val = dict(opt['datasets']['val_vis'], prompts=os.path.join(REF, opt['datasets']['val_vis']['prompts']))
    ds = PromptDataset(val)
    assert len(ds) > 0 and ds[0]['latents'].shape == tuple(val['latent_size'])
    word = list(train_cfg['replace_mapping'].values())[0].split(' ')[0]
    assert word in ds[0]['prompts'] and '<TOK>' not in ds[0]['prompts']
    # one optimisation step runs on this recipe's model block (tiny preset, emulated kernels)
    from tests.test_host_cpu import _batch
    b = _batch()
    b['prompts'] = [f'a {list(train_cfg["replace_mapping"].values())[0]} in the park'] * 2
    out = engine.step(b)
    assert torch.isfinite(out['loss'])


@pytest.mark.parametrize('path', TEST, ids=[os.path.basename(p)[:28] for p in TEST])
def test_reference_test_recipe_loads(path):
    from mixofshow.utils.options import load_options
    opt = load_options(path)
    assert set(opt) <= TOP_KEYS and 'lora_path' in opt['path'] and opt['val']['sample']['num_inference_steps'] == 50
    # (1001_EDLoRA_hina...yml carries a stray `alpha_list` inside `models`; the entry point reads val.alpha_list, like the reference)
    assert set(opt['models']) <= MODEL_KEYS | {'alpha_list'}
