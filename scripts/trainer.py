"""Counterpart of the reference's src/trainer.py: same hard-coded hyper-parameter surface, same call sequence
(load_indexes -> PatchHandler3D.initialize_dataset -> TrainerController -> init_model_dir -> train_network).
Launch with `python -m torch.distributed.run --nproc-per-node N scripts/trainer.py` for data-parallel training.

The input pipeline is the measured one: DevicePatchHandler3D keeps the decoded HDF5 volumes in HBM and cuts / rotates / normalises
every batch on the device (bit-identical to the host loader, tests/test_gpu_device_loader.py).  FDN_HOST_LOADER=1 selects the host
loader instead -- PatchHandler3D with its prefetch thread, worker pool and pinned staging buffers -- e.g. when the dataset does
not fit beside the activations."""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
data = importlib.import_module("4dflownet_amd.data")
parallel = importlib.import_module("4dflownet_amd.parallel")
trainer = importlib.import_module("4dflownet_amd.trainer")


def make_handler(data_dir, patch_size, res_increase, batch_size, mask_threshold, resynthesize=None):
    """(handler, kwargs for initialize_dataset): the on-device loader unless FDN_HOST_LOADER is set.  resynthesize (device loader only):
    see DevicePatchHandler3D."""
    if os.environ.get("FDN_HOST_LOADER", "0") not in ("", "0"):
        if resynthesize is not None:
            raise ValueError("resynthesize needs the on-device loader (unset FDN_HOST_LOADER)")
        return data.PatchHandler3D(data_dir, patch_size, res_increase, batch_size, mask_threshold), {"pinned": True}
    data_device = importlib.import_module("4dflownet_amd.data_device")
    extra = {} if resynthesize is None else {"resynthesize": resynthesize}
    return data_device.DevicePatchHandler3D(data_dir, patch_size, res_increase, batch_size, mask_threshold, **extra), {}


if __name__ == "__main__":
    data_dir = os.environ.get("FDN_DATA_DIR", '../data')
    training_file = '{}/train.csv'.format(data_dir)
    validate_file = '{}/validate.csv'.format(data_dir)
    QUICKSAVE = True
    benchmark_file = '{}/benchmark.csv'.format(data_dir)
    restore = False
    if restore:
        model_dir = "../models/4DFlowNet"
        model_file = "4DFlowNet-best.h5"

    # Hyperparameters optimisation variables (trainer.py:28-39)
    initial_learning_rate = 2e-4
    epochs = 60
    batch_size = 20
    accum_steps = 1          # optimiser step = accum_steps consecutive batches of batch_size (x ranks); 1 = the reference's schedule
    # None = train on the low-res volumes of the files; dict(seed=s) = every epoch the training set's low-res volumes are synthesised anew
    # on the device from the high-res ones (fresh noise, SNR, VENCs and magnitude level; DevicePatchHandler3D(resynthesize=...))
    resynthesize = None
    mask_threshold = 0.6
    network_name = '4DFlowNet'
    patch_size = 16
    res_increase = 2
    low_resblock = 8
    hi_resblock = 4
    # fine-tuning: None = every layer trains; "hires" (hi-res ResBlocks + heads), "heads", or a list of layer names freeze the rest
    # (TrainerController(trainable=...), the same as `layer.trainable = False` in Keras).  Together with `restore` the run starts from the
    # restored WEIGHTS with a fresh optimiser: the saved slots belong to the variables that were trainable then.
    trainable = None
    # loss and heads (TrainerController.py:23-24 and the manuscript's bounded heads): weight of the divergence term, weight of the non-fluid
    # region in both terms (1 = the reference's shipped loss, 0 = fluid only), output activation of the heads (None / 'linear' | 'tanh')
    div_weight = 0
    non_fluid_weight = 1
    output_activation = None
    # penalty of the data term: 'mse' (the reference's calculate_mse) | 'mae' | 'huber' (loss_param = delta, None = 1.0; on velocities
    # normalised to [-1, 1] choose a smaller one) | 'charbonnier' (loss_param = epsilon, None = 1e-3).  The divergence term stays squared;
    # train_mse / val_mse and val_loss are then in the chosen loss's units.  Whether one of them beats 'mse' is unmeasured.
    loss = 'mse'
    loss_param = None

    parallel.init_from_env()
    trainset = data.load_indexes(training_file)
    valset = data.load_indexes(validate_file)
    z, kw = make_handler(data_dir, patch_size, res_increase, batch_size, mask_threshold, resynthesize=resynthesize)
    trainset = z.initialize_dataset(trainset, shuffle=True, n_parallel=None, **kw)
    valdh, kw = make_handler(data_dir, patch_size, res_increase, batch_size, mask_threshold)
    valset = valdh.initialize_dataset(valset, shuffle=True, n_parallel=None, **kw)
    testset = None
    if QUICKSAVE and benchmark_file is not None:
        benchmark_set = data.load_indexes(benchmark_file)
        ph, kw = make_handler(data_dir, patch_size, res_increase, batch_size, mask_threshold)
        testset = ph.initialize_dataset(benchmark_set, shuffle=False, shard=(0, 1), **kw)

    print("4DFlowNet Patch %d, lr %s, batch %d" % (patch_size, initial_learning_rate, batch_size))
    network = trainer.TrainerController(patch_size, res_increase, initial_learning_rate, QUICKSAVE, network_name,
                                        low_resblock, hi_resblock, accum_steps=accum_steps, trainable=trainable, div_weight=div_weight,
                                        non_fluid_weight=non_fluid_weight, output_activation=output_activation, loss=loss,
                                        loss_param=loss_param)
    network.init_model_dir()
    if restore and trainable is not None:
        print("Fine-tuning from the weights of %s..." % model_file)
        network.model.load_weights("%s/%s" % (model_dir, model_file))
    elif restore:
        print("Restoring model %s..." % model_file)
        network.restore_model(model_dir, model_file)
        print("Learning rate", network.optimizer.lr)
    network.train_network(trainset, valset, n_epoch=epochs, testset=testset)
